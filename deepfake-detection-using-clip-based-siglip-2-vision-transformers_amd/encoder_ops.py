"""PyTorch custom ops over the encoder's C ABI (SURVEY.md §8b "Who calls it"): torch.ops.siglip_hip.encoder_fwd /
encoder_bwd, with fake (meta) implementations and a registered autograd formula, so that torch.compile(fullgraph=True)
of the SURROUNDING model (cifake_binary_classifier.py:1888, hidf_video_classifier.py:2922) traces straight through the
encoder call without a graph break.  The ops are thin: they allocate outputs through PyTorch and make the ctypes calls;
what lives between calls belongs to the owners in ``encoder_state`` that the module (found by its handle) holds.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Optional, Sequence

import torch

from . import lib as _lib
from .encoder_state import OPERAND_DTYPE

_MODULES: "weakref.WeakValueDictionary[int, torch.nn.Module]" = weakref.WeakValueDictionary()
_NEXT_HANDLE = [1]


def register(module) -> int:
    """A fresh op handle for ``module`` (a ``SiglipVisionModelHIP``): ops take the handle, not the module."""
    handle = _NEXT_HANDLE[0]
    _NEXT_HANDLE[0] += 1
    _MODULES[handle] = module
    return handle


def _module_of(handle: int):
    mod = _MODULES.get(int(handle))
    if mod is None:
        raise RuntimeError(f"siglip_hip: encoder handle {handle} is not alive (module was deleted)")
    return mod


def _geometry(cfg, H, W, B=None, rows=None):
    """(B, H, W, N, M, grid) of a call on H x W images: N tokens per image, M = B * N rows.  The batch is given, or
    follows from the rows of a token-major buffer."""
    gh, gw = H // cfg.patch_size, W // cfg.patch_size
    N = gh * gw
    if B is None:
        B = rows // N
    return B, H, W, N, B * N, (gh, gw)


def _input_geometry(cfg, pixel_values, layout=0, img_h=0, img_w=0):
    """``_geometry`` of a forward's input, which is checked."""
    P = cfg.patch_size
    if layout == 2:   # ready patch-major operand [B*N, Kp] (preprocess.to_patch_operand); geometry travels beside it
        N = _geometry(cfg, img_h, img_w, 0)[3]
        kp = (3 * P * P + 63) // 64 * 64
        if pixel_values.dim() != 2 or pixel_values.shape[1] != kp or N == 0 or pixel_values.shape[0] % N:
            raise ValueError(f"patch operand must be (B*{N}, {kp}), got {tuple(pixel_values.shape)}")
        return _geometry(cfg, img_h, img_w, rows=pixel_values.shape[0])
    if pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
        raise ValueError(f"pixel_values must be (B,3,H,W), got {tuple(pixel_values.shape)}")
    B, _, H, W = pixel_values.shape
    if H < P or W < P:
        raise ValueError(f"image size ({H},{W}) is smaller than patch_size {P}")
    return _geometry(cfg, H, W, B)


def _slot_plan(tap_ids, train, L):
    """Which buffer each of the L + 1 hidden-state slots of sgl_forward_slots uses: (n_rest, plan), plan[l] = (True, i) for
    the tensor of the i-th entry of tap_ids (distinct), (False, k) for row k of hs_rest [n_rest, B*N, D].  Training keeps
    every hidden state, so each slot nobody asked for has a row of its own; inference ping-pongs between two rows
    (neighbours differ in parity)."""
    tapset = {int(t): i for i, t in enumerate(tap_ids)}
    n_rest = (L + 1 - len(tapset)) if train else min(2, L + 1 - len(tapset))
    plan, k = [], 0
    for l in range(L + 1):
        if l in tapset:
            plan.append((True, tapset[l]))
        elif train:
            plan.append((False, k))
            k += 1
        else:
            plan.append((False, l & 1))
    return n_rest, plan


@torch.library.custom_op("siglip_hip::encoder_fwd", mutates_args=())
def encoder_fwd(pixel_values: torch.Tensor, params: Sequence[torch.Tensor], handle: int, train: bool, interp: bool,
                want_pooled: bool, tap_ids: Sequence[int], first_trainable: int, layout: int, img_h: int,
                img_w: int, recompute: bool = False) -> List[torch.Tensor]:
    """sgl_forward_slots.  Returns [pooled (B,D) or empty, last_hidden_state (B,N,D), one (B,N,D) tensor per entry of
    tap_ids (distinct, ascending), saved (uint8 activation arena, empty when not training), hs_rest (the hidden-state
    slots nobody asked for: [n, B*N, D])].  No output aliases another.  recompute (training only): run on the module's
    recompute context, which saves no per-block activations (its backward recomputes them)."""
    mod = _module_of(handle)
    cfg = mod.config
    L, D = cfg.num_hidden_layers, cfg.hidden_size
    lib = _lib.load()
    px = pixel_values
    channels_last = 0
    if layout == 2:
        want = OPERAND_DTYPE[mod.compute_dtype]
        if px.dtype != want or not px.is_contiguous():
            raise ValueError(f"patch operand must be contiguous {want} (the encoder's compute dtype)")
        channels_last = 2
    else:
        if px.dtype != torch.float32:
            px = px.float()
        if not px.is_contiguous():
            if px.is_contiguous(memory_format=torch.channels_last):
                channels_last = 1
            else:
                px = px.contiguous()
    B, H, W, N, M, grid = _input_geometry(cfg, px, layout, img_h, img_w)
    if grid != (cfg.native_grid, cfg.native_grid) and not interp:
        raise ValueError(f"Input image size ({H}*{W}) doesn't match model native "
                         f"({cfg.image_size}*{cfg.image_size}); pass interpolate_pos_encoding=True")
    dev = px.device
    recompute = bool(recompute) and train     # inference ignores the policy
    with torch.cuda.device(dev):
        shadow, weights = mod._shadows.prepared(dev, params)
        sizes = mod._contexts.sizes(B, H, W, train, recompute)
        taps = [torch.empty((B, N, D), dtype=torch.float32, device=dev) for _ in tap_ids]
        n_rest, plan = _slot_plan(tap_ids, train, L)
        hs_rest = torch.empty((n_rest, M, D), dtype=torch.float32, device=dev)
        slots = (_lib._fp * (L + 1))()
        for l, (is_tap, i) in enumerate(plan):
            slots[l] = (taps[i] if is_tap else hs_rest[i]).data_ptr()
        last = torch.empty((B, N, D), dtype=torch.float32, device=dev)
        pooled = torch.empty((B, D) if want_pooled else (0,), dtype=torch.float32, device=dev)
        saved = torch.empty(sizes[1] if train else 0, dtype=torch.uint8, device=dev)
        # a plain training forward leaves the workspace alone; a recompute one writes its block region there
        ws = mod._contexts.workspace(sizes[2], dev) if (recompute or not train) else None
        ctx = mod._contexts.get(recompute)
        st = lib.sgl_forward_slots(ctx, C.byref(weights), shadow.data_ptr(), px.data_ptr(), channels_last, B, H, W,
                                   1 if interp else 0, slots, last.data_ptr(),
                                   pooled.data_ptr() if want_pooled else None, saved.data_ptr() if train else None,
                                   sizes[1] if train else 0, _lib.ptr(ws), 0 if ws is None else sizes[2],
                                   int(first_trainable), _lib.current_stream_handle(dev))
        _lib.check(st, "sgl_forward_slots", ctx)
    if train:
        mod._shadows.note_forward(saved)
        mod._grads.note_forward()
    return [pooled, last, *taps, saved, hs_rest]


@encoder_fwd.register_fake
def _(pixel_values, params, handle, train, interp, want_pooled, tap_ids, first_trainable, layout, img_h, img_w,
      recompute=False):
    mod = _module_of(handle)
    cfg = mod.config
    L, D = cfg.num_hidden_layers, cfg.hidden_size
    B, H, W, N, M, _ = _input_geometry(cfg, pixel_values, layout, img_h, img_w)
    if not all(isinstance(v, int) for v in (B, H, W)):
        raise RuntimeError("siglip_hip::encoder_fwd needs static image shapes under torch.compile (dynamic=False)")
    new = pixel_values.new_empty
    n_rest, _ = _slot_plan(tap_ids, train, L)
    saved_bytes = mod._contexts.sizes(B, H, W, True, bool(recompute))[1] if train else 0
    return [new((B, D) if want_pooled else (0,), dtype=torch.float32), new((B, N, D), dtype=torch.float32),
            *[new((B, N, D), dtype=torch.float32) for _ in tap_ids], new((saved_bytes,), dtype=torch.uint8),
            new((n_rest, M, D), dtype=torch.float32)]


def _contiguous_f32(g):
    if g is None:
        return None
    g = g.float() if g.dtype != torch.float32 else g
    return g.contiguous()


@torch.library.custom_op("siglip_hip::encoder_bwd", mutates_args=())
def encoder_bwd(grads: Sequence[Optional[torch.Tensor]], taps: Sequence[torch.Tensor], saved: torch.Tensor,
                hs_rest: torch.Tensor, params: Sequence[torch.Tensor], handle: int, image_hw: Sequence[int],
                interp: bool, want_pooled: bool, tap_ids: Sequence[int], needs: Sequence[bool],
                recompute: bool = False, want_px: bool = False, px_channels_last: bool = False) -> List[torch.Tensor]:
    """sgl_backward_begin_pa -> sgl_backward_layer_pa (L-1 ... first trainable block) -> sgl_backward_embed, on the context
    of the policy the forward ran with (recompute: each sgl_backward_layer_pa recomputes its block first).  The request
    argument of the two is NULL (the plain _p step) unless a ``capture_attention_gradients`` of the module is active.
    grads = [d pooled, d last_hidden_state, d tap...] (None = no gradient).  Returns the flat fp32 gradient chunks of
    ``GradPlan.layout(needs)`` (the DDP all-reduce units); the autograd formula slices the per-parameter views out of
    them outside the op, so no output of the op aliases another.
    want_px: the input requires a gradient.  Every block L-1 ... 0 then runs with need_dx = 1 (frozen ones with NULL
    destinations), sgl_backward_embed_px replaces sgl_backward_embed, and d_pixels (B,3,H,W) fp32, in channels_last memory
    format when px_channels_last, is one more output after the chunks (no chunk when the whole encoder is frozen)."""
    mod = _module_of(handle)
    lib = _lib.load()
    cfg = mod.config
    L = cfg.num_hidden_layers
    # hs_rest is [n, B*N, D], also when every slot is a tap (n = 0)
    B, H, W = _geometry(cfg, int(image_hw[0]), int(image_hw[1]), rows=hs_rest.shape[1])[:3]
    dev = saved.device
    table, plan, shadows, contexts = mod._table, mod._grads, mod._shadows, mod._contexts
    shadows.check_backward(saved)
    params = table.params()

    d_pooled = _contiguous_f32(grads[0]) if want_pooled else None
    d_last = _contiguous_f32(grads[1])
    tap_grads = [None] * (L + 1)
    hs_ptr = [None] * (L + 1)
    for l, (is_tap, i) in enumerate(_slot_plan(tap_ids, True, L)[1]):
        hs_ptr[l] = (taps[i] if is_tap else hs_rest[i]).data_ptr()
        if is_tap:
            tap_grads[l] = _contiguous_f32(grads[2 + i])

    with torch.cuda.device(dev):
        # 1. the plan and its buffers
        chunks, groups = plan.layout(needs)
        flats = plan.buffers(chunks, params, dev)
        # 2. the grads struct (the C side skips the pooling head, and the post-LN when d_last is None too, without d_pooled)
        g, g_keep = plan.grads_struct(chunks, flats, groups.get("head", ()) if d_pooled is None else ())
        # 3. the reducer decides, once per autograd pass, whether chunks are handed over from here (ddp.py)
        reducer = plan.reducer
        overlapped = reducer is not None and reducer.backward_node(
            [(total, [(params[i], off, n) for i, off, n in entries]) for total, _, entries in chunks])
        ready = {members[-1]: flat for flat, (_, members, _) in zip(flats, chunks)} if overlapped else {}

        def group_done(grp):
            """Hand a chunk to the reducer once its last group (in completion order) is complete."""
            if grp in ready:
                reducer.reduce_bucket(ready[grp])

        # 4. head, blocks L-1 ... stop, embeddings
        train_emb = "emb" in groups
        first = min((l for l in range(L) if table.block_label[l] in groups), default=L)
        stop = 0 if (train_emb or want_px) else first
        sizes = contexts.sizes(B, H, W, True, bool(recompute))
        ws = contexts.workspace(sizes[2], dev)
        stream = _lib.current_stream_handle(dev)
        _, wts, shadow = shadows.binding()
        cx = contexts.get(bool(recompute))
        # an active capture_attention_gradients: the steps it wants a map from carry a request (NULL: the plain step)
        cap = plan.capture
        heads, N = cfg.num_attention_heads, hs_rest.shape[1] // B

        def attn_grad_request(step):
            if cap is None or (step == L and d_pooled is None):
                return None, None
            return cap.request(step, B, heads, N, dev)

        amap, req = attn_grad_request(L)
        st = lib.sgl_backward_begin_pa(cx, C.byref(wts), shadow.data_ptr(), C.byref(g), B, H, W, hs_ptr[L],
                                       _lib.ptr(d_last), _lib.ptr(d_pooled), _lib.ptr(tap_grads[L]), saved.data_ptr(),
                                       sizes[1], ws.data_ptr(), sizes[2], stream, C.byref(req) if req else None)
        _lib.check(st, "sgl_backward_begin_pa", cx)
        if req:
            cap.delivered(L, amap)
        group_done("head")
        for l in range(L - 1, stop - 1, -1):
            need_dx = 1 if (l > stop or train_emb or want_px) else 0
            amap, req = attn_grad_request(l)
            st = lib.sgl_backward_layer_pa(cx, C.byref(wts), shadow.data_ptr(), C.byref(g), l, B, H, W, hs_ptr[l],
                                           _lib.ptr(tap_grads[l]), need_dx, saved.data_ptr(), sizes[1], ws.data_ptr(),
                                           sizes[2], stream, C.byref(req) if req else None)
            _lib.check(st, f"sgl_backward_layer_pa[{l}]", cx)
            if req:
                cap.delivered(l, amap)
            group_done(table.block_label[l])
        d_pixels = None
        if want_px:
            d_pixels = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev,
                                   memory_format=torch.channels_last if px_channels_last else torch.contiguous_format)
            nbytes = C.c_size_t()
            _lib.check(lib.sgl_query_input_grad_bytes(cx, B, H, W, C.byref(nbytes)), "sgl_query_input_grad_bytes", cx)
            px_scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
            st = lib.sgl_backward_embed_px(cx, C.byref(wts), C.byref(g), B, H, W, 1 if interp else 0,
                                           d_pixels.data_ptr(), 1 if px_channels_last else 0, px_scratch.data_ptr(),
                                           nbytes.value, saved.data_ptr(), sizes[1], ws.data_ptr(), sizes[2], stream)
            _lib.check(st, "sgl_backward_embed_px", cx)
        elif train_emb:
            st = lib.sgl_backward_embed(cx, C.byref(wts), C.byref(g), B, H, W, 1 if interp else 0,
                                        saved.data_ptr(), sizes[1], ws.data_ptr(), sizes[2], stream)
            _lib.check(st, "sgl_backward_embed", cx)
        if train_emb:
            group_done("emb")
        # 5. the reducer waits for what it was handed
        if overlapped:
            reducer.finish()
    # 6. the chunks (and d_pixels) are the op's outputs
    return flats + ([d_pixels] if want_px else [])


@encoder_bwd.register_fake
def _(grads, taps, saved, hs_rest, params, handle, image_hw, interp, want_pooled, tap_ids, needs, recompute=False,
      want_px=False, px_channels_last=False):
    mod = _module_of(handle)
    chunks, _ = mod._grads.layout(needs)
    outs = [saved.new_empty((total,), dtype=torch.float32) for total, _, _ in chunks]
    if want_px:
        B, H, W = _geometry(mod.config, int(image_hw[0]), int(image_hw[1]), rows=hs_rest.shape[1])[:3]
        outs.append(saved.new_empty((B, 3, H, W), dtype=torch.float32).contiguous(
            memory_format=torch.channels_last if px_channels_last else torch.contiguous_format))
    return outs


def _encoder_setup_context(ctx, inputs, output):
    pixel_values, params, handle, train, interp, want_pooled, tap_ids, first_trainable, layout, img_h, img_w = inputs[:11]
    ctx.set_materialize_grads(False)
    # the backward runs with the policy its forward ran with, whatever model.recompute says by then
    ctx.recompute = bool(inputs[11])
    ctx.handle, ctx.interp, ctx.want_pooled, ctx.tap_ids = handle, interp, want_pooled, list(tap_ids)
    ctx.image_hw = [int(img_h), int(img_w)] if layout == 2 else [int(pixel_values.shape[2]), int(pixel_values.shape[3])]
    ctx.ntaps, ctx.nparams, ctx.train = len(tap_ids), len(params), train
    # d_pixels comes back in the input's dtype and memory format (the storage the forward read when it is fp32)
    ctx.px_dtype = pixel_values.dtype
    ctx.px_channels_last = bool(layout != 2 and pixel_values.dim() == 4 and not pixel_values.is_contiguous()
                                and pixel_values.is_contiguous(memory_format=torch.channels_last))
    if train:
        # saving the taps (outputs) makes autograd's version counter catch a consumer's in-place edit of a hidden state
        ctx.save_for_backward(*output[2:], *params)
        # hidden_states[i] only feeds gradient to the embeddings and to blocks < i: with those frozen
        # (Siglip2sidafrozen.py:757-768) the tap's gradient would be computed by the consumer (the SID decoder's tap
        # projections) and then dropped here, so tell autograd not to ask for it
        dead = [t for i, t in zip(tap_ids, output[2:2 + len(tap_ids)]) if first_trainable > 0 and i <= first_trainable]
        dead += [output[-2], output[-1]] + ([] if want_pooled else [output[0]])
        ctx.mark_non_differentiable(*dead)


def _encoder_backward(ctx, grads):
    if not ctx.train:
        raise RuntimeError("siglip_hip::encoder_fwd was run with train=False: nothing was saved for backward")
    saved_t = ctx.saved_tensors
    nt = ctx.ntaps
    taps, saved, hs_rest, params = list(saved_t[:nt]), saved_t[nt], saved_t[nt + 1], list(saved_t[nt + 2:])
    needs = [bool(n) for n in ctx.needs_input_grad[1]] if isinstance(ctx.needs_input_grad[1], (list, tuple)) \
        else [p.requires_grad for p in params]
    want_px = bool(ctx.needs_input_grad[0])
    if want_px and torch.is_grad_enabled():
        raise RuntimeError("SiglipVisionModelHIP: double backward (create_graph=True) through d loss / d pixel_values is "
                           "not supported: the HIP backward is not itself differentiable; take first-order gradients "
                           "(create_graph=False), or use finite differences of them for a Hessian-vector product")
    flats = torch.ops.siglip_hip.encoder_bwd(list(grads[:2 + nt]), taps, saved, hs_rest, params, ctx.handle, ctx.image_hw,
                                             ctx.interp, ctx.want_pooled, ctx.tap_ids, needs, ctx.recompute, want_px,
                                             ctx.px_channels_last)
    d_pixels = None
    if want_px:
        d_pixels = flats[-1] if ctx.px_dtype == torch.float32 else flats[-1].to(ctx.px_dtype)
        flats = flats[:-1]
    chunks, _ = _module_of(ctx.handle)._grads.layout(needs)
    pgrads: List[Optional[torch.Tensor]] = [None] * len(params)
    for flat, (_, _, entries) in zip(flats, chunks):
        for i, off, n in entries:
            pgrads[i] = flat[off:off + n].view(params[i].shape)
    # pytree structure of the inputs: an EMPTY int list is a list node, a non-empty one a leaf (torch/_library/autograd.py)
    # one entry per argument the caller passed (needs_input_grad has that structure): 11, or 12 with recompute
    return (d_pixels, pgrads, None, None, None, None, ([] if len(ctx.tap_ids) == 0 else None), None, None, None, None) + \
        (None,) * (len(ctx.needs_input_grad) - 11)


encoder_fwd.register_autograd(_encoder_backward, setup_context=_encoder_setup_context)


_OPERAND_CODE = {torch.float32: _lib.SGL_DTYPE_F32, torch.bfloat16: _lib.SGL_DTYPE_BF16, torch.float16: _lib.SGL_DTYPE_F16}


def ragged_geometry(cfg, images):
    """[(gh, gw)] of a ragged batch, the images as (3, H, W) views; the checks need no device work."""
    if isinstance(images, torch.Tensor) or len(images) == 0:
        raise ValueError("forward_ragged takes a non-empty sequence of (3,H,W) or (1,3,H,W) tensors, one per image; "
                         "a (B,3,H,W) batch of one size goes through model(pixel_values=...)")
    P = cfg.patch_size
    views, grids = [], []
    for i, x in enumerate(images):
        if x.dim() == 4 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 3 or x.shape[0] != 3:
            raise ValueError(f"image {i} must be (3,H,W) or (1,3,H,W), got {tuple(x.shape)}")
        if x.shape[1] < P or x.shape[2] < P:
            raise ValueError(f"image {i}: size ({x.shape[1]},{x.shape[2]}) is smaller than patch_size {P}")
        views.append(x)
        grids.append((x.shape[1] // P, x.shape[2] // P))
    return views, grids


def forward_ragged(mod, views, grids, tap_ids: Sequence[int]):
    """sgl_forward_ragged on images of different sizes: each goes through sgl_op_im2col (B = 1) into its rows of one packed
    patch operand [T, Kp], then one encoder call.  Returns (pooled (S,D) or None, last_hidden_state (T,D), one (T,D) tensor
    per entry of tap_ids (distinct, ascending)).  Inference only; the outputs are outside autograd.  Not a custom op: a graph
    break under torch.compile."""
    cfg = mod.config
    L, D, P = cfg.num_hidden_layers, cfg.hidden_size, cfg.patch_size
    lib = _lib.load()
    dev = views[0].device
    S = len(views)
    lens = [gh * gw for gh, gw in grids]
    T = sum(lens)
    kp = (3 * P * P + 63) // 64 * 64
    op_dtype = OPERAND_DTYPE[mod.compute_dtype]
    with torch.cuda.device(dev):
        params = mod._table.params()
        shadow, weights = mod._shadows.prepared(dev, params)
        ws_bytes = mod._contexts.ragged_sizes(grids)     # refuses a bad batch before anything is enqueued
        ws = mod._contexts.workspace(ws_bytes, dev)
        stream = _lib.current_stream_handle(dev)
        operand = torch.empty((T, kp), dtype=op_dtype, device=dev)
        row = 0
        for x, n in zip(views, lens):
            x = x.detach()
            if x.dtype != torch.float32:
                x = x.float()
            x = x.contiguous()
            st = lib.sgl_op_im2col(x.data_ptr(), 0, operand[row:].data_ptr(), _OPERAND_CODE[op_dtype], 1, x.shape[1],
                                   x.shape[2], P, kp, stream)
            _lib.check(st, "sgl_op_im2col")
            row += n
        taps = [torch.empty((T, D), dtype=torch.float32, device=dev) for _ in tap_ids]
        n_rest, plan = _slot_plan(tap_ids, False, L)
        hs_rest = torch.empty((n_rest, T, D), dtype=torch.float32, device=dev)
        slots = (_lib._fp * (L + 1))()
        for l, (is_tap, i) in enumerate(plan):
            slots[l] = (taps[i] if is_tap else hs_rest[i]).data_ptr()
        last = torch.empty((T, D), dtype=torch.float32, device=dev)
        pooled = torch.empty((S, D), dtype=torch.float32, device=dev) if mod.use_head else None
        flat = (C.c_int * (2 * S))(*[v for g in grids for v in g])
        ctx = mod._contexts.get(False)
        st = lib.sgl_forward_ragged(ctx, C.byref(weights), shadow.data_ptr(), operand.data_ptr(), flat, S, slots,
                                    last.data_ptr(), _lib.ptr(pooled), ws.data_ptr(), ws_bytes, stream)
        _lib.check(st, "sgl_forward_ragged", ctx)
    return pooled, last, taps


def attention_maps(mod, saved: torch.Tensor, B: int, H: int, W: int, layers: Sequence[int], head_mean: bool):
    """sgl_attention_probs for each entry of ``layers`` (block index, or L for the pooling head) on the activation arena
    ``saved`` of a saving forward of ``mod`` at (B, H, W): fresh fp32 tensors, (B,heads,N,N) / (B,heads,N) each, without
    the heads dimension when ``head_mean``.  The arena is only read.  Not a custom op (a graph break under torch.compile):
    the tensors are outside autograd."""
    lib = _lib.load()
    cfg = mod.config
    L, heads = cfg.num_hidden_layers, cfg.num_attention_heads
    N = _geometry(cfg, H, W, B)[3]
    dev = saved.device
    mode = _lib.ATTN_PROBS_HEAD_MEAN if head_mean else _lib.ATTN_PROBS_FULL
    lead = (B,) if head_mean else (B, heads)
    outs = []
    with torch.cuda.device(dev):
        ctx = mod._contexts.get(False)
        stream = _lib.current_stream_handle(dev)
        for l in layers:
            out = torch.empty(lead + ((N,) if l == L else (N, N)), dtype=torch.float32, device=dev)
            st = lib.sgl_attention_probs(ctx, B, H, W, saved.data_ptr(), saved.numel(), int(l), mode, out.data_ptr(),
                                         out.numel() * 4, stream)
            _lib.check(st, f"sgl_attention_probs[{l}]", ctx)
            outs.append(out)
    return outs
