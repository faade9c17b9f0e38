"""What a ``SiglipVisionModelHIP`` keeps between calls, one owner per concern (the module itself holds only these):

``ParamTable``      the parameters in C-ABI order, built once from one spec (ABI field -> HF attribute path);
``Contexts``        the C contexts (plain / recompute), the ``sgl_query_sizes`` cache and the workspace; destroys the
                    contexts when it dies, which is the only place they are destroyed;
``WeightShadows``   the shadow arena, what it is current for, the weights struct, and which generation a forward used;
``GradPlan``        the gradient chunk layout, the flat buffers behind it and the grads struct; and, while one is
                    active, the ``AttnGradCapture`` the next backward writes attention-gradient maps for.

None of them is copied or pickled with the module: a copy gets fresh ones (``SiglipVisionModelHIP.__copy__``).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import lib as _lib

# compute_dtype -> sgl_config.compute_dtype, and the dtype of the patch-GEMM operand (``patches=``) each mode reads
COMPUTE_DTYPES = {"bf16": _lib.SGL_DTYPE_BF16, "fp32": _lib.SGL_DTYPE_F32, "bf16x3": _lib.SGL_DTYPE_BF16X3,
                  "fp16": _lib.SGL_DTYPE_F16, "mxfp8": _lib.SGL_DTYPE_MXFP8}
# mxfp8 keeps the patch embedding in bf16 (only the four block GEMMs read MX-fp8 operands)
OPERAND_DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32, "bf16x3": torch.float32, "fp16": torch.float16,
                 "mxfp8": torch.bfloat16}
# modes without a backward: a forward that would have to save activations for one is refused
INFERENCE_ONLY = {"mxfp8"}


# ---------------------------------------------------------------------------------------------------------
# the parameter table
# ---------------------------------------------------------------------------------------------------------
# ABI field -> attribute path below the module (below ``encoder.layers[l]`` for a block), in struct order
_EMB = {"patch_w": "embeddings.patch_embedding.weight", "patch_b": "embeddings.patch_embedding.bias",
        "pos": "embeddings.position_embedding.weight"}
_BLOCK = {"ln1_w": "layer_norm1.weight", "ln1_b": "layer_norm1.bias",
          "q_w": "self_attn.q_proj.weight", "q_b": "self_attn.q_proj.bias",
          "k_w": "self_attn.k_proj.weight", "k_b": "self_attn.k_proj.bias",
          "v_w": "self_attn.v_proj.weight", "v_b": "self_attn.v_proj.bias",
          "o_w": "self_attn.out_proj.weight", "o_b": "self_attn.out_proj.bias",
          "ln2_w": "layer_norm2.weight", "ln2_b": "layer_norm2.bias",
          "fc1_w": "mlp.fc1.weight", "fc1_b": "mlp.fc1.bias", "fc2_w": "mlp.fc2.weight", "fc2_b": "mlp.fc2.bias"}
_POST_LN = {"post_ln_w": "post_layernorm.weight", "post_ln_b": "post_layernorm.bias"}
_HEAD = {"probe": "head.probe", "in_proj_w": "head.attention.in_proj_weight", "in_proj_b": "head.attention.in_proj_bias",
         "out_proj_w": "head.attention.out_proj.weight", "out_proj_b": "head.attention.out_proj.bias",
         "head_ln_w": "head.layernorm.weight", "head_ln_b": "head.layernorm.bias",
         "head_fc1_w": "head.mlp.fc1.weight", "head_fc1_b": "head.mlp.fc1.bias",
         "head_fc2_w": "head.mlp.fc2.weight", "head_fc2_b": "head.mlp.fc2.bias"}
assert list(_BLOCK) == _lib.LAYER_FIELDS and list(_HEAD) == _lib.HEAD_FIELDS
for _struct in (_lib.SglWeights, _lib.SglGrads):
    assert [n for n, _ in _struct._fields_ if n not in ("layers", "accumulate")] == [*_EMB, *_POST_LN, *_HEAD]

# fields with a 16-bit (or split) copy in the shadow arena: per block, then the globals
_SHADOWED = {"q_w", "k_w", "v_w", "q_b", "k_b", "v_b", "o_w", "fc1_w", "fc1_b", "fc2_w",
             "patch_w", "in_proj_w", "out_proj_w", "head_fc1_w", "head_fc1_b", "head_fc2_w"}


class Entry(NamedTuple):
    label: str              # gradient group: "emb", "layer7", "head" (the post-LN rides with the head)
    block: Optional[int]    # transformer block, None outside the blocks
    unit: int               # weight-shadow unit: the block, or L for everything else
    field: str              # member of SglLayerPtrs (blocks) or SglWeights / SglGrads
    path: str               # attribute path below the module (= state_dict key without ``vision_model.``)
    owner: nn.Module        # the sub-module holding the parameter ...
    attr: str               # ... under this name


class ParamTable:
    """The module's parameters in the order of the C structs.  ``params()`` reads the live ``Parameter`` objects out of
    their owners' ``_parameters``, so a replaced Parameter is seen; callers fetch once per forward / backward and hand
    the list down."""

    def __init__(self, module: nn.Module, num_layers: int, use_head: bool):
        self.L = num_layers
        self.block_label = [f"layer{l}" for l in range(num_layers)]       # gradient group of block l
        self.labels = ["emb", *self.block_label, "head"]
        spec = [("emb", None, f, p) for f, p in _EMB.items()]
        for l in range(num_layers):
            spec += [(self.block_label[l], l, f, f"encoder.layers.{l}.{p}") for f, p in _BLOCK.items()]
        spec += [("head", None, f, p) for f, p in {**_POST_LN, **(_HEAD if use_head else {})}.items()]
        self.entries = tuple(
            Entry(label, block, num_layers if block is None else block, field, path,
                  module.get_submodule(path.rpartition(".")[0]), path.rpartition(".")[2])
            for label, block, field, path in spec)
        self.n_emb = len(_EMB)
        self.patch_w = [e.field for e in self.entries].index("patch_w")

    def params(self):
        return [e.owner._parameters[e.attr] for e in self.entries]

    def fill(self, struct, ptr_of):
        """An ``SglWeights`` / ``SglGrads`` whose member for entry i is ``ptr_of(i)``; returns it with the
        ``SglLayerPtrs`` array it points into (keep both alive)."""
        layers = (_lib.SglLayerPtrs * max(self.L, 1))()
        s = struct()
        s.layers = C.cast(layers, C.POINTER(_lib.SglLayerPtrs))
        for i, e in enumerate(self.entries):
            setattr(s if e.block is None else layers[e.block], e.field, ptr_of(i))
        return s, layers


# ---------------------------------------------------------------------------------------------------------
# contexts, sizes, workspace
# ---------------------------------------------------------------------------------------------------------
class Contexts:
    """The C context of each activation policy in use (created on first use), what ``sgl_query_sizes`` said, and the
    workspace.  The shadow arena's layout does not depend on the policy, so the shadows (and FusedAdamW's binding of
    them) live on the plain context."""

    def __init__(self, cfg, compute_dtype: str, use_head: bool):
        self.cfg, self.compute_dtype, self.use_head = cfg, compute_dtype, use_head
        self._plain = self._recompute = None
        self._sizes = {}
        self._ws = None

    def get(self, recompute: bool = False):
        if self._plain is None or (recompute and self._recompute is None):
            lib = _lib.load()
            cfg = self.cfg
            c = _lib.SglConfig(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                               cfg.patch_size, cfg.native_grid, cfg.layer_norm_eps, COMPUTE_DTYPES[self.compute_dtype],
                               1 if self.use_head else 0)
            if self._plain is None:
                ctx = lib.sgl_create(C.byref(c))
                if not ctx:
                    raise _lib.SglError(f"sgl_create: unsupported configuration {cfg}")
                self._plain = ctx
            if recompute and self._recompute is None:
                ctx = lib.sgl_create_ex(C.byref(c), _lib.SGL_RECOMPUTE_BLOCKS)
                if not ctx:
                    raise _lib.SglError(f"sgl_create_ex: recompute unsupported for {cfg} ({self.compute_dtype})")
                self._recompute = ctx
                P = cfg.patch_size
                sh = [C.c_size_t(), C.c_size_t()]
                for cx, out in zip((self._plain, ctx), sh):
                    _lib.check(lib.sgl_query_sizes(cx, 1, P, P, 0, C.byref(out), None, None), "sgl_query_sizes", cx)
                assert sh[0].value == sh[1].value, "shadow arena layout must not depend on the recompute policy"
        return self._recompute if recompute else self._plain

    def sizes(self, B, H, W, train, recompute=False):
        """(shadow, saved, workspace) bytes of ``sgl_query_sizes``, cached."""
        key = (B, H, W, bool(train), bool(recompute))
        if key not in self._sizes:
            ctx = self.get(bool(recompute))
            a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
            st = _lib.load().sgl_query_sizes(ctx, B, H, W, 1 if train else 0, C.byref(a), C.byref(b), C.byref(c))
            _lib.check(st, "sgl_query_sizes", ctx)
            self._sizes[key] = (a.value, b.value, c.value)
        return self._sizes[key]

    def ragged_sizes(self, grids):
        """Workspace bytes of ``sgl_query_sizes_ragged`` for a ragged batch of these (gh, gw) grids, cached."""
        key = ("ragged", tuple(grids))
        if key not in self._sizes:
            if len(self._sizes) > 4096:     # every new mix of sizes is a new key
                self._sizes.clear()
            ctx = self.get(False)
            flat = (C.c_int * (2 * len(grids)))(*[v for g in grids for v in g])
            n = C.c_size_t()
            st = _lib.load().sgl_query_sizes_ragged(ctx, flat, len(grids), C.byref(n))
            _lib.check(st, "sgl_query_sizes_ragged", ctx)
            self._sizes[key] = n.value
        return self._sizes[key]

    def workspace(self, nbytes, dev):
        """Scratch reused across calls (stream-ordered; the C side only needs it intact within one forward / backward)."""
        ws = self._ws
        if ws is None or ws.device != dev or ws.numel() < nbytes:
            self._ws = ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return ws

    def drop_workspace(self):
        self._ws = None

    def __del__(self):
        try:
            for ctx in (self._plain, self._recompute):
                if ctx is not None and _lib._lib is not None:
                    _lib._lib.sgl_destroy(ctx)
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------
# weight shadows
# ---------------------------------------------------------------------------------------------------------
class WeightShadows:
    """The arena of 16-bit (or split) weight copies the kernels read, and its bookkeeping: one (data_ptr, _version) key
    per parameter, grouped per unit (block l, or L for everything else), says what the arena is current for; ``serial``
    counts its generations (one per refresh, one per adoption of shadows the optimizer wrote)."""

    def __init__(self, table: ParamTable, contexts: Contexts):
        self.table, self.contexts = table, contexts
        self.arena = None
        self.keys = None
        self.serial = 0
        self._weights = None        # (SglWeights, its SglLayerPtrs array, dense patch_w copy or None)
        self._weights_key = None
        self._forwards = {}         # saved-arena pointer of a training forward -> serial it ran with

    def invalidate(self, release: bool = False):
        """Nothing in the arena is current any more: the next forward re-casts every unit.  release: the parameters
        themselves moved (``nn.Module._apply``), so the arena and the weights struct go as well."""
        self.keys = None
        if release:
            self.arena = self._weights = None

    def _unit_keys(self, params):
        keys = [[] for _ in range(self.table.L + 1)]
        for e, p in zip(self.table.entries, params):
            keys[e.unit].append((p.data_ptr(), p._version))
        return [tuple(k) for k in keys]

    def _weights_struct(self, params):
        for e, p in zip(self.table.entries, params):
            # the 4-D patch-conv weight may be channels_last after model.to(memory_format=torch.channels_last)
            # (Siglip2sidafrozen.py:1191): only the shadow refresh reads it, through a contiguous copy (prepared)
            strided_ok = e.field == "patch_w" and p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last)
            if p.dtype != torch.float32 or not (p.is_contiguous() or strided_ok):
                raise RuntimeError("encoder master parameters must be contiguous fp32 (the HIP path keeps its own "
                                   "16-bit shadows); do not call .half()/.bfloat16() on the encoder")
        return [*self.table.fill(_lib.SglWeights, lambda i: params[i].data_ptr()), None]

    def prepared(self, dev, params):
        """(shadow arena, weights struct), refreshed when any master parameter changed (optimizer step,
        load_state_dict, EMA swap of ``param.data`` — ``cifake_binary_classifier.py:227-236``)."""
        lib = _lib.load()
        ctx = self.contexts.get()
        if params[0].device != dev:
            raise RuntimeError(f"model is on {params[0].device}, input on {dev}")
        ptr_key = tuple(p.data_ptr() for p in params)
        if self._weights is None or self._weights_key != ptr_key:
            self._weights, self._weights_key = self._weights_struct(params), ptr_key
        weights = self._weights[0]
        # only what changed is re-cast, so a frozen-prefix run (Siglip2sidafrozen.py:757-768) refreshes its 6 trainable
        # blocks, not all 27
        L = self.table.L
        keys = self._unit_keys(params)
        fresh = self.arena is None or self.arena.device != dev or self.keys is None
        if fresh or self.keys != keys:
            P = self.contexts.cfg.patch_size
            nbytes = self.contexts.sizes(1, P, P, False)[0]
            if self.arena is None or self.arena.device != dev or self.arena.numel() < nbytes:
                self.arena = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                fresh = True
            if fresh:
                dirty, glob = None, 1
            else:
                dirty = bytes(1 if keys[l] != self.keys[l] else 0 for l in range(L))
                glob = 1 if keys[L] != self.keys[L] else 0
            pw = params[self.table.patch_w]
            if glob and not pw.is_contiguous():
                self._weights[2] = pw.detach().contiguous()          # kept alive until the next refresh
                weights.patch_w = self._weights[2].data_ptr()
            st = lib.sgl_prepare_weights_dirty(ctx, C.byref(weights), self.arena.data_ptr(), self.arena.numel(), dirty,
                                               glob, _lib.current_stream_handle(dev))
            _lib.check(st, "sgl_prepare_weights_dirty", ctx)
            self.keys = keys
            self.serial += 1
        return self.arena, weights

    def binding(self):
        """What ``FusedAdamW`` binds its shadow destinations to: (plain context, weights struct, arena), or None before
        the first forward."""
        if self.arena is None:
            return None
        return self.contexts.get(), self._weights[0], self.arena

    def units_in_sync(self):
        """Per block (and, last entry, the globals): is the shadow arena current for the parameters as they are now?"""
        if self.arena is None or self.keys is None:
            return None
        return [a == b for a, b in zip(self._unit_keys(self.table.params()), self.keys)]

    def adopt(self, was_in_sync, written_ptrs):
        """Called by ``FusedAdamW`` after a step that wrote the shadows of the parameters in ``written_ptrs`` in its own
        pass: a unit that was in sync before the step, and whose shadowed parameters were all either written or left
        untouched, is in sync again — adopt the new versions so the next forward does not re-cast it."""
        if was_in_sync is None or self.keys is None:
            return
        params = self.table.params()
        now = self._unit_keys(params)
        n_units = self.table.L + 1
        changed_ok = [True] * n_units
        pos = [0] * n_units
        for e, p in zip(self.table.entries, params):
            old = self.keys[e.unit][pos[e.unit]]
            pos[e.unit] += 1
            if (p.data_ptr(), p._version) != old and e.field in _SHADOWED and p.data_ptr() not in written_ptrs:
                changed_ok[e.unit] = False
        adopted = False
        for u in range(n_units):
            if was_in_sync[u] and changed_ok[u] and now[u] != self.keys[u]:
                self.keys[u] = now[u]
                adopted = True
        if adopted:
            self.serial += 1

    def note_forward(self, saved):
        """Remember which generation a training forward used (checked by its backward)."""
        if len(self._forwards) > 64:
            self._forwards.clear()
        self._forwards[saved.data_ptr()] = self.serial

    def check_backward(self, saved):
        serial = self._forwards.get(saved.data_ptr())
        if serial is not None and serial != self.serial:
            raise RuntimeError(
                "SiglipVisionModelHIP: parameters changed between this forward and its backward (optimizer step, EMA "
                "swap or load_state_dict in between re-cast the bf16 weight shadows); run backward before touching them")


# ---------------------------------------------------------------------------------------------------------
# gradient memory plan
# ---------------------------------------------------------------------------------------------------------
def _taper(order, max_chunks):
    """Cut the completion-ordered group list into at most ``max_chunks`` runs whose lengths shrink towards the END: the
    exchange of the last chunk overlaps nothing (backward is over when it starts), the first has the whole backward to
    hide behind.  Boundaries, counted from the end, follow j(j+1)/2 (28 groups, 8 chunks -> 6,6,4,4,3,3,1,1); the small
    embeddings group rides with the block it follows."""
    tail = [order[-1]] if len(order) > 1 and order[-1] == "emb" else []
    body = order[:len(order) - len(tail)]
    n, c = len(body), max(1, min(max_chunks, len(body)))
    tri = c * (c + 1) // 2
    cuts = sorted({n - min(n, max(j, round(n * j * (j + 1) / 2 / tri))) for j in range(1, c)} | {0, n})
    runs = [body[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    if tail:
        if runs:
            runs[-1] = runs[-1] + tail
        else:
            runs = [tail]
    return runs


class GradPlan:
    """Where a backward's parameter gradients go: the chunk layout, the flat buffers behind it, the ``SglGrads`` that
    points into them, and the reducer (a ``ddp.GradBucketReducer`` or None) whose ``max_buckets`` sets the chunk count."""

    def __init__(self, table: ParamTable):
        self.table = table
        self.reducer = None
        self.capture = None         # the active AttnGradCapture (capture_attention_gradients), consulted by encoder_bwd
        self._layouts = {}
        self._buffers = {}
        self._forwards = 0          # training forwards so far: a buffer is not reused within one autograd pass

    def set_reducer(self, reducer):
        self.reducer = reducer
        self.drop_buffers()

    def drop_buffers(self):
        self._buffers = {}

    def note_forward(self):
        self._forwards += 1

    def layout(self, needs):
        """Pure function of (which parameters need gradients, chunk count): the gradient memory plan, memoized, so the op,
        its fake implementation and the autograd formula of one backward share one result.

        Groups (embeddings, each block, post-LN + head) are listed in the order the backward completes them (head, block
        L-1 ... first trainable block, embeddings) and cut into at most ``max_buckets`` chunks of consecutive groups; every
        chunk is ONE flat fp32 tensor (= one DDP collective, ddp.py) holding its groups' per-parameter gradients, each
        16-byte aligned.  Returns (chunks, groups): chunks = [(total_elems, [group names], [(param index, offset, numel)])],
        groups = {group name: [param indices]}."""
        max_buckets = self.reducer.max_buckets if self.reducer is not None else 8
        key = (tuple(map(bool, needs)), max_buckets)
        if key in self._layouts:
            return self._layouts[key]
        entries, params = self.table.entries, self.table.params()
        groups: dict[str, list[int]] = {}
        for idx, e in enumerate(entries):
            if needs[idx]:
                groups.setdefault(e.label, []).append(idx)
        order = [g for g in reversed(self.table.labels) if g in groups]
        # q/k/v weight (and bias) gradients back to back: the C side then runs them as one dW GEMM / one column sum
        rank = {"q_w": 0, "k_w": 1, "v_w": 2, "q_b": 3, "k_b": 4, "v_b": 5}
        chunks = []
        for members in _taper(order, max(1, max_buckets)):
            off, placed = 0, []
            for grp in members:
                for i in sorted(groups[grp], key=lambda i: (rank.get(entries[i].field, 6), i)):
                    n = params[i].numel()
                    placed.append((i, off, n))
                    off += (n + 3) // 4 * 4
            chunks.append((off, members, placed))
        self._layouts[key] = chunks, groups
        return chunks, groups

    def buffers(self, chunks, params, dev):
        """The flat tensors of ``layout``.  The C side overwrites every element, so they are reused from step to
        step (no memset, stable pointers for FusedAdamW's device table) — but only when that is provably safe: no
        parameter's .grad still aliases the cached tensor (gradient accumulation, zero_grad(set_to_none=False)) AND a
        training forward has run since the backward that last filled it (two backward invocations of this module inside
        ONE autograd pass — siamese use, a loss summed over two forward calls — must not share memory: the first one's
        gradients may not have been accumulated yet).  Otherwise this backward gets fresh memory."""
        flats = []
        for ci, (total, members, entries) in enumerate(chunks):
            key = (ci, tuple(members), tuple(e[0] for e in entries))
            hit = self._buffers.get(key)
            flat = None
            if hit is not None and hit[0].device == dev and hit[0].numel() == total and hit[1] != self._forwards:
                flat = hit[0]
                base, end = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
                if any(params[i].grad is not None and base <= params[i].grad.data_ptr() < end for i, _, _ in entries):
                    flat = None
            if flat is None:
                flat = torch.empty(total, dtype=torch.float32, device=dev)
            if hit is None or hit[1] != self._forwards:
                self._buffers[key] = (flat, self._forwards)
            flats.append(flat)
        return flats

    def grads_struct(self, chunks, flats, zero):
        """The ``SglGrads`` (accumulate = 0) over ``flats``: NULL for a parameter without a slot.  The slots of the
        parameter indices in ``zero`` are cleared first (groups the C side will not write in this call)."""
        slot = [None] * len(self.table.entries)
        for flat, (_, _, entries) in zip(flats, chunks):
            for i, off, n in entries:
                slot[i] = flat[off:off + n]
        for i in zero:
            slot[i].zero_()
        g, layers = self.table.fill(_lib.SglGrads, lambda i: _lib.ptr(slot[i]))
        g.accumulate = 0
        return g, layers


# ---------------------------------------------------------------------------------------------------------
# attention-gradient capture
# ---------------------------------------------------------------------------------------------------------
ATTN_GRAD_KINDS = {"grad": _lib.ATTN_GRAD_DP, "prob_grad": _lib.ATTN_GRAD_PDP, "relevance": _lib.ATTN_GRAD_RELEVANCE}


class AttnGradCapture:
    """What ``SiglipVisionModelHIP.capture_attention_gradients`` returns: a context manager round a forward + backward.
    While it is active, ``encoder_bwd`` asks it for a request per backward step (``request``) and tells it when the
    step's call is enqueued (``delivered``).  Afterwards ``maps[layer]`` holds the map of each requested block the
    backward reached, (B,N,N) or (B,heads,N,N), and ``pooling`` the pooling head's, (B,N) or (B,heads,N) (None when the
    model has no head or the score did not go through ``pooler_output``).  With ``sink`` the blocks share ONE buffer:
    ``sink(layer, tensor)`` is called after each block's call is enqueued (blocks arrive in descending order, on the
    current stream) and must consume the tensor before returning control to the backward: the next block overwrites it."""

    def __init__(self, plan, num_layers: int, layers, head_mean: bool, kind: int, sink=None):
        self._plan, self.L = plan, num_layers
        self.layers, self.head_mean, self.kind, self.sink = list(layers), head_mean, kind, sink
        self.mode = _lib.ATTN_PROBS_HEAD_MEAN if head_mean else _lib.ATTN_PROBS_FULL
        self.maps, self.pooling = {}, None
        self._wanted = set(self.layers)
        self._seen = set()
        self._buf = None

    def __enter__(self):
        if self._plan.capture is not None:
            raise RuntimeError("capture_attention_gradients: another capture is already active on this model")
        self._plan.capture = self
        return self

    def __exit__(self, exc_type, exc, tb):
        self._plan.capture = None
        self._buf = None
        if exc_type is None:
            missing = sorted(self._wanted - self._seen)
            if missing:
                raise RuntimeError(
                    f"capture_attention_gradients: the backward never reached block(s) {missing}: blocks below the first "
                    "trainable one get no gradient unless the input does; call pixel_values.requires_grad_() before the "
                    "forward (model.attention_relevance does), or request only blocks that train")
        return False

    def request(self, layer: int, B: int, heads: int, N: int, dev):
        """(tensor, SglAttnGradReq) for backward step ``layer`` (L: the pooling head), or (None, None)."""
        pool = layer == self.L
        if not pool and layer not in self._wanted:
            return None, None
        shape = ((B,) if self.head_mean else (B, heads)) + ((N,) if pool else (N, N))
        if self.sink is not None and not pool:
            if self._buf is None or self._buf.shape != shape or self._buf.device != dev:
                self._buf = torch.empty(shape, dtype=torch.float32, device=dev)
            out = self._buf
        else:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        return out, _lib.SglAttnGradReq(out.data_ptr(), out.numel() * 4, self.kind, self.mode)

    def delivered(self, layer: int, out: torch.Tensor) -> None:
        if layer == self.L:
            self.pooling = out
            return
        self._seen.add(layer)
        if self.sink is not None:
            self.sink(layer, out)
        else:
            self.maps[layer] = out
