"""Host-side mirror of the two call surfaces the reference uses for the encoder, backed by the
hand-written gfx950 kernels in ``libsiglip_hip.so``.

Surface H (HuggingFace-style; ``Siglip2sidafrozen.py:753,757-768,771,787-793``):
    ``SiglipVisionModelHIP.from_pretrained(path_or_name)``, ``model(pixel_values=..., output_hidden_states=True,
    interpolate_pos_encoding=True)`` → ``.pooler_output`` / ``.last_hidden_state`` / ``.hidden_states``;
    ``output_attentions=True`` → ``.attentions`` / ``.pooling_attention`` (detached), ``model.attention_rollout(x)``;
    ``model.capture_attention_gradients()`` round a forward + backward, ``model.attention_relevance(x, score_fn)``;
    ``.config.hidden_size``; ``.vision_model.embeddings`` / ``.vision_model.encoder.layers[i]`` for freezing;
    ``state_dict`` keys equal HF ``SiglipVisionModel`` keys.
Surface O (open_clip-style; ``cifake_binary_classifier.py:625-638,721``, ``hidf_video_classifier.py:259-273,307``):
    ``create_model_and_transforms(name, pretrained, device)`` → ``(model, None, preprocess)``;
    ``model.encode_image(x)`` → un-normalised (B, D); ``model.embed_dim``.

PyTorch is plumbing only (device memory, streams, autograd graph).  All arithmetic of the encoder runs in the
HIP library; there is no CPU fallback — calling the model on a CPU tensor raises.

This module holds the two surfaces only.  The calls into the library are the custom ops of ``encoder_ops``
(``torch.ops.siglip_hip.encoder_fwd`` / ``encoder_bwd``); what a model keeps between calls (parameter table, C contexts,
weight shadows, gradient memory plan) belongs to the owners of ``encoder_state``, one instance of each per model.
"""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import encoder_ops
from .config import SiglipVisionConfig, get_config, NAMED_CONFIGS
from .encoder_state import (COMPUTE_DTYPES, OPERAND_DTYPE, INFERENCE_ONLY,  # noqa: F401  (part of this module's surface)
                            Contexts, GradPlan, ParamTable, WeightShadows)
from .weights import seeded_state_dict


# ---------------------------------------------------------------------------------------------------------
# parameter holders: same module tree / names as HF SiglipVisionModel (TF:modeling_siglip.py:116-135,
# 253-271,309-316,324-331,560-571,622-631) so state_dict keys and the reference's freezing code line up
# ---------------------------------------------------------------------------------------------------------
class _Affine(nn.Module):
    def __init__(self, out_f, in_shape=None, bias=True):
        super().__init__()
        shape = (out_f,) if in_shape is None else (out_f, *in_shape)
        self.weight = nn.Parameter(torch.zeros(shape))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_f))


class _AttnParams(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.k_proj = _Affine(d, (d,))
        self.v_proj = _Affine(d, (d,))
        self.q_proj = _Affine(d, (d,))
        self.out_proj = _Affine(d, (d,))


class _MLPParams(nn.Module):
    def __init__(self, d, i):
        super().__init__()
        self.fc1 = _Affine(i, (d,))
        self.fc2 = _Affine(d, (i,))


class _LayerParams(nn.Module):
    def __init__(self, d, i):
        super().__init__()
        self.layer_norm1 = _Affine(d)
        self.self_attn = _AttnParams(d)
        self.layer_norm2 = _Affine(d)
        self.mlp = _MLPParams(d, i)


class _EncoderParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_LayerParams(cfg.hidden_size, cfg.intermediate_size)
                                     for _ in range(cfg.num_hidden_layers)])


class _EmbeddingParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.patch_embedding = _Affine(cfg.hidden_size, (3, cfg.patch_size, cfg.patch_size))
        self.position_embedding = _Affine(cfg.num_positions, (cfg.hidden_size,), bias=False)


class _MHAParams(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.zeros(3 * d, d))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d))
        self.out_proj = _Affine(d, (d,))


class _HeadParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        d = cfg.hidden_size
        self.probe = nn.Parameter(torch.zeros(1, 1, d))
        self.attention = _MHAParams(d)
        self.layernorm = _Affine(d)
        self.mlp = _MLPParams(d, cfg.intermediate_size)


@dataclass
class VisionModelOutput:
    """Fields of HF ``BaseModelOutputWithPooling`` the reference reads (``Siglip2sidafrozen.py:788-793``)."""
    last_hidden_state: torch.Tensor
    pooler_output: Optional[torch.Tensor]
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    # output_attentions=True only (after the fields above, so positional construction and indexing keep their meaning)
    attentions: Optional[Tuple[torch.Tensor, ...]] = None
    pooling_attention: Optional[torch.Tensor] = None

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output, self.hidden_states)[i]


@dataclass
class RaggedVisionModelOutput:
    """What ``forward_ragged`` returns for S images of different sizes.  Token-major tensors are PACKED: image i owns rows
    ``cu_seqlens[i] : cu_seqlens[i + 1]`` (its ``grids[i][0] * grids[i][1]`` patches in row-major order), T rows in all,
    no padding."""
    last_hidden_state: torch.Tensor                           # (T, D)
    pooler_output: Optional[torch.Tensor]                     # (S, D); None without the pooling head
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None  # (T, D) each
    grids: Tuple[Tuple[int, int], ...] = ()                   # (gh_i, gw_i)
    cu_seqlens: Tuple[int, ...] = (0,)                        # S + 1 row offsets (host integers)

    def unpack(self, t: torch.Tensor):
        """The S per-image views (n_i, D) of a packed (T, D) tensor."""
        if t.shape[0] != self.cu_seqlens[-1]:
            raise ValueError(f"expected a packed tensor of {self.cu_seqlens[-1]} rows, got {tuple(t.shape)}")
        return [t[a:b] for a, b in zip(self.cu_seqlens[:-1], self.cu_seqlens[1:])]

    def token_grid(self, t: torch.Tensor, i: int):
        """Image i's tokens of a packed (T, D) tensor as a (gh_i, gw_i, D) view."""
        gh, gw = self.grids[i]
        return self.unpack(t)[i].view(gh, gw, t.shape[-1])


# ---------------------------------------------------------------------------------------------------------
# surface H
# ---------------------------------------------------------------------------------------------------------
def _hf_state_dict_hook(module, state_dict, prefix, local_metadata):
    """state_dict(): parameters are registered without the ``vision_model.`` level; add it on the way out."""
    for k in [k for k in state_dict if k.startswith(prefix) and not k.startswith(prefix + "vision_model.")]:
        state_dict[prefix + "vision_model." + k[len(prefix):]] = state_dict.pop(k)


def _hf_load_pre_hook(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    """load_state_dict(): strip the ``vision_model.`` level (also when this module is nested in a parent)."""
    pv = prefix + "vision_model."
    for k in [k for k in state_dict if k.startswith(pv)]:
        state_dict[prefix + k[len(pv):]] = state_dict.pop(k)


def vision_tower_only(state_dict: dict) -> dict:
    """Keep the vision tower of a full SiglipModel checkpoint: keys under ``vision_model.`` when that level exists (the
    published google/siglip* files also carry ``text_model.*``, ``logit_scale``, ``logit_bias``), everything otherwise."""
    if any(k.startswith("vision_model.") for k in state_dict):
        return {k: v for k, v in state_dict.items() if k.startswith("vision_model.")}
    return {k: v for k, v in state_dict.items()
            if not (k.startswith("text_model.") or k in ("logit_scale", "logit_bias"))}


class SiglipVisionModelHIP(nn.Module):
    """Drop-in for ``transformers.SiglipVisionModel`` on the reference's path (see module docstring)."""

    def __init__(self, config, compute_dtype: str = "bf16", recompute: bool = False):
        super().__init__()
        self.config = get_config(config)
        # "bf16": the benchmarked mode (bf16 MFMA operands, fp32 accumulate / residual stream / statistics);
        # "fp32": strict reference arithmetic (plain fp32 FMAs, no matrix cores): tightest parity, slow;
        # "bf16x3": strict mode on the matrix cores (every GEMM as one bf16 MFMA GEMM over hi/lo-split operands, fp32
        #           accumulate; ~2^-17 relative per product): the north-star "logits within 1e-3" at MFMA speed;
        # "fp16": "bf16" with fp16 operands and weight shadows (fp16 MFMA, same kernels and speed, 3 more mantissa bits):
        #         the arithmetic of a torch.autocast(float16) run; operand overflow gives inf (GradScaler sees it);
        # "mxfp8": INFERENCE ONLY: "bf16" with the four projection GEMMs of every block on MX-fp8 operands (e4m3 with one
        #          power-of-two scale per 32 inputs, twice the bf16 MFMA rate); for inference and frozen-backbone training
        #          (heads train on its detached features); a forward that would differentiate the encoder raises
        # recompute=True: gradient checkpointing (see the ``recompute`` property)
        if compute_dtype not in COMPUTE_DTYPES:
            raise ValueError("compute_dtype must be 'bf16', 'fp32', 'bf16x3', 'fp16' or 'mxfp8'")
        self.compute_dtype = compute_dtype
        self._recompute = False
        self.recompute = recompute
        cfg = self.config
        self.embeddings = _EmbeddingParams(cfg)
        self.encoder = _EncoderParams(cfg)
        self.post_layernorm = _Affine(cfg.hidden_size)
        self.use_head = bool(cfg.vision_use_head)
        if self.use_head:
            self.head = _HeadParams(cfg)
        self._gradient_checkpointing = False
        self._new_runtime()
        # checkpoints keep transformers' key names (``vision_model.encoder.layers.N…``, Siglip2sidafrozen.py:1639)
        self._register_state_dict_hook(_hf_state_dict_hook)
        self._register_load_state_dict_pre_hook(_hf_load_pre_hook)

    # ---- HF surface ------------------------------------------------------------------------------------
    @property
    def vision_model(self):
        """transformers-4.x layout alias used by the reference's freezing code
        (``Siglip2sidafrozen.py:757,762``): ``encoder.vision_model.embeddings`` / ``.encoder.layers``."""
        return self

    @property
    def recompute(self) -> bool:
        """Activation policy of training forwards (gradient checkpointing).  False (default): every block's activations are
        kept until the backward.  True: only the hidden states are kept and the backward recomputes each block from its
        input (one extra LN1 .. fc1 per block, about a fifth of the step; bitwise the same gradients), so activation
        memory drops to about a sixth.  Applies from the next forward; a backward always uses its forward's policy.
        Inference forwards ignore it."""
        return self._recompute

    @recompute.setter
    def recompute(self, value: bool) -> None:
        if not isinstance(value, bool):
            raise TypeError(f"recompute must be a bool, got {type(value).__name__}")
        if value and self.compute_dtype in INFERENCE_ONLY:
            raise ValueError(f"compute_dtype={self.compute_dtype!r} is inference-only: there is no backward to recompute for")
        self._recompute = value

    @classmethod
    def from_pretrained(cls, name_or_path: str, compute_dtype: str = "bf16", seed: int = 0,
                        allow_random_init: bool = False, recompute: bool = False):
        """Local directory (``config.json`` + ``model.safetensors``) or a known config name.  A published
        google/siglip(2) checkpoint is the FULL SiglipModel (``vision_model.*``, ``text_model.*``, ``logit_scale``,
        ``logit_bias``): like ``SiglipVisionModel.from_pretrained`` (Siglip2sidafrozen.py:753) only the vision tower is
        kept.  There is no network: a bare name has no weights to load, which is an error unless
        ``allow_random_init=True`` asks for the closed-form seeded initialisation (``weights.seeded_state_dict``)."""
        if os.path.isdir(name_or_path):
            with open(os.path.join(name_or_path, "config.json")) as f:
                raw = json.load(f)
            raw = raw.get("vision_config", raw)
            fields = SiglipVisionConfig.__dataclass_fields__
            cfg = SiglipVisionConfig(**{k: v for k, v in raw.items() if k in fields})
            model = cls(cfg, compute_dtype, recompute)
            from safetensors.torch import load_file
            model.load_state_dict(vision_tower_only(load_file(os.path.join(name_or_path, "model.safetensors"))))
            return model
        if name_or_path in NAMED_CONFIGS:
            if not allow_random_init:
                raise OSError(
                    f"'{name_or_path}' names an architecture, not a local checkpoint directory, and there is no network "
                    "to fetch pretrained weights from.  Pass a directory holding config.json + model.safetensors, or "
                    "allow_random_init=True to get SEEDED RANDOM weights of that architecture (benchmarks / tests).")
            warnings.warn(f"SiglipVisionModelHIP.from_pretrained('{name_or_path}'): no checkpoint — using seeded RANDOM "
                          "weights (allow_random_init=True); outputs are not those of the pretrained model",
                          stacklevel=2)
            model = cls(get_config(name_or_path), compute_dtype, recompute)
            model.load_state_dict(seeded_state_dict(model.config, seed))
            return model
        raise OSError(f"{name_or_path} is neither a local checkpoint directory nor a known config name "
                      f"(no network access); known: {sorted(NAMED_CONFIGS)}")

    def gradient_checkpointing_enable(self, recompute: bool = False, **_):
        """``recompute=True`` turns block recompute on (``self.recompute = True``).  The bare call, as the reference makes
        it (``Siglip2sidafrozen.py:1195-1196``, on a frozen-prefix config where recompute only costs time), is accepted for
        interface parity but does nothing, and says so once: activations of a 128-image so400m batch fit the 288 GB of
        HBM3E, so nothing is recomputed unless asked for."""
        if recompute:
            self.recompute = True
            return
        if not self._gradient_checkpointing:
            warnings.warn("SiglipVisionModelHIP.gradient_checkpointing_enable(): no-op — the HIP encoder keeps all "
                          "activations (0.82 GB per so400m@384 image; 288 GB HBM3E) and does not recompute; pass "
                          "recompute=True (or set model.recompute = True) to trade compute for memory", stacklevel=2)
        self._gradient_checkpointing = True

    def gradient_checkpointing_disable(self):
        """Turn block recompute off (``self.recompute = False``)."""
        self.recompute = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts HF names with or without the ``vision_model.`` prefix, or an open_clip/timm vision tower
        (``…visual.trunk.blocks.N.attn.qkv.weight``, converted by ``weights_io.timm_to_hf``)."""
        from . import weights_io
        if weights_io.detect_format(state_dict.keys()) == "timm":
            state_dict = weights_io.encoder_state_from_checkpoint(state_dict, self.config)
        return super().load_state_dict(dict(state_dict), strict=strict, **kw)

    def forward(self, pixel_values=None, output_hidden_states: bool = False, interpolate_pos_encoding: bool = False,
                hidden_state_ids=None, patches=None, output_attentions: bool = False, attention_layers=None,
                attention_heads: str = "all", **_):
        """Traceable by Dynamo: everything device-side happens inside ``torch.ops.siglip_hip.encoder_fwd``.
        ``patches`` (a ``preprocess.PatchOperand``) replaces ``pixel_values``: the resized + normalised images already
        in the patch GEMM's operand layout, so neither an fp32 (B,3,S,S) tensor nor the im2col pass exists.

        ``output_attentions=True`` adds ``.attentions``: one fp32 tensor per block of ``attention_layers`` (default: every
        block, as HF), (B,heads,N,N) each, or (B,N,N), the mean over heads, with ``attention_heads="mean"`` (all full maps
        of so400m@384 are 27 x 34 MB per image: ask for the layers, or the mean, you need), and ``.pooling_attention``: the
        pooling head's probe attention (B,heads,N), or (B,N) with ``"mean"``, when the model has its head.  The maps are
        recomputed by a HIP kernel from the q, k and log-sum-exp the saving forward keeps; every other output, and every
        gradient, is bit-identical to the same call without the flag.  Unlike HF's, the maps are DETACHED: no gradient
        flows through them.  Works in every grad mode (under ``no_grad`` the call runs the saving forward and drops the
        arena afterwards); not on a ``recompute=True`` model and not with ``compute_dtype="mxfp8"`` (RuntimeError).  The
        call is a graph break under ``torch.compile``; without the flag nothing changes."""
        if output_attentions:
            return self._forward_with_attentions(pixel_values, output_hidden_states, interpolate_pos_encoding,
                                                 hidden_state_ids, patches, attention_layers, attention_heads)
        return self._run(pixel_values, output_hidden_states, interpolate_pos_encoding, hidden_state_ids, patches)[0]

    def _attention_request(self, attention_layers, attention_heads):
        """(block indices, head_mean) of an ``output_attentions=True`` call, checked before any device work."""
        L = self.config.num_hidden_layers
        if self._recompute:
            raise RuntimeError("output_attentions=True on a recompute=True model: recompute keeps no per-block q, k to "
                               "rebuild the maps from; use a model without recompute for attention maps")
        if self.compute_dtype in INFERENCE_ONLY:
            raise RuntimeError(f"output_attentions=True with compute_dtype={self.compute_dtype!r}: the inference-only mode "
                               "has no saving forward; use compute_dtype='bf16' / 'fp16' / 'bf16x3' / 'fp32' for attention maps")
        if attention_heads not in ("all", "mean"):
            raise ValueError(f"attention_heads must be 'all' or 'mean', got {attention_heads!r}")
        layers = list(range(L)) if attention_layers is None else [int(i) for i in attention_layers]
        for i in layers:
            if not -L <= i < L:
                raise RuntimeError(f"attention_layers entry {i} is out of range for {L} blocks; valid: {-L} .. {L - 1} "
                                   "(the pooling head's map is .pooling_attention)")
        return [i % L for i in layers], attention_heads == "mean"

    @torch.compiler.disable
    def _forward_with_attentions(self, pixel_values, output_hidden_states, interpolate_pos_encoding, hidden_state_ids,
                                 patches, attention_layers, attention_heads):
        layers, head_mean = self._attention_request(attention_layers, attention_heads)
        out, saved, (B, H, W) = self._run(pixel_values, output_hidden_states, interpolate_pos_encoding, hidden_state_ids,
                                          patches, keep_arena=True)
        maps = encoder_ops.attention_maps(self, saved, B, H, W, layers + ([self.config.num_hidden_layers]
                                                                        if self.use_head else []), head_mean)
        out.attentions = tuple(maps[:len(layers)])
        out.pooling_attention = maps[-1] if self.use_head else None
        return out

    def attention_rollout(self, pixel_values, residual: float = 0.5, interpolate_pos_encoding: bool = True):
        """Attention rollout (``heads.attention_rollout``) of every block's head-mean map, read through the pooling head's
        probe attention: one relevance value per patch, (B, gh, gw), detached.  One saving forward; the per-head (B,H,N,N)
        maps are never materialised."""
        from .heads import attention_rollout
        if not self.use_head:
            raise RuntimeError("attention_rollout reads the rollout through the pooling head's probe attention and this "
                               "model has none; use heads.attention_rollout(model(..., output_attentions=True, "
                               "attention_heads='mean').attentions) for the (B,N,N) rollout")
        with torch.no_grad():
            out = self(pixel_values=pixel_values, interpolate_pos_encoding=interpolate_pos_encoding,
                       output_attentions=True, attention_heads="mean")
            r = attention_rollout(out.attentions, residual, pooling=out.pooling_attention)
        P = self.config.patch_size
        return r.view(r.shape[0], pixel_values.shape[-2] // P, pixel_values.shape[-1] // P)

    @torch.compiler.disable
    def capture_attention_gradients(self, layers=None, heads: str = "mean", kind: str = "relevance", sink=None):
        """Context manager round a forward + backward of this model: the backward also writes, per requested block, the
        gradient of whatever was differentiated with respect to the block's attention probabilities P, formed by a HIP
        kernel at the one point of the backward where q, k, v, the log-sum-exp and dO all exist.  ``kind``: ``"grad"``
        (dScore/dP, what HF's eager ``attentions[l].grad`` holds), ``"prob_grad"`` (P * dScore/dP) or ``"relevance"``
        (its relu; a NaN stays NaN).  ``heads``: ``"mean"`` gives (B,N,N) per block (the per-head tensor never exists),
        ``"all"`` (B,heads,N,N).  ``layers``: block indices (negative ones count from the end; default: every block).

            with model.capture_attention_gradients() as cap:
                model(pixel_values=x.requires_grad_()).pooler_output[:, 1].sum().backward()
            cap.maps[layer], cap.pooling

        ``cap.pooling`` is the pooling head's map, (B,N) / (B,heads,N), when the score went through ``pooler_output``.
        With ``sink(layer, tensor)`` one buffer is reused: the sink is called after each block's kernel is enqueued,
        blocks in descending order, and ``cap.maps`` stays empty.  The maps are detached; every gradient the backward
        produces is bit-identical with and without the capture.  At exit a requested block the backward never reached
        (a frozen prefix without an input gradient) raises RuntimeError.  Not on a ``recompute=True`` model and not with
        ``compute_dtype="mxfp8"`` (RuntimeError).  A graph break under ``torch.compile``."""
        from .encoder_state import ATTN_GRAD_KINDS, AttnGradCapture
        if self._recompute:
            raise RuntimeError("capture_attention_gradients on a recompute=True model: recompute keeps no per-block q, k to "
                               "rebuild the maps from; use a model without recompute for attention gradients")
        if self.compute_dtype in INFERENCE_ONLY:
            raise RuntimeError(f"capture_attention_gradients with compute_dtype={self.compute_dtype!r}: the inference-only "
                               "mode has no backward; use compute_dtype='bf16' / 'fp16' / 'bf16x3' / 'fp32' for attention "
                               "gradients")
        if kind not in ATTN_GRAD_KINDS:
            raise ValueError(f"kind must be one of {sorted(ATTN_GRAD_KINDS)}, got {kind!r}")
        blocks, head_mean = self._attention_request(layers, heads)
        return AttnGradCapture(self._grads, self.config.num_hidden_layers, blocks, head_mean, ATTN_GRAD_KINDS[kind], sink)

    @torch.compiler.disable
    def attention_relevance(self, pixel_values, score_fn, interpolate_pos_encoding: bool = True):
        """Class-specific relevance of every patch for ``score_fn(VisionModelOutput) -> (B,)`` or a scalar (e.g.
        ``lambda o: head(o.pooler_output)[:, 1]``): gradient-weighted attention relevance (``heads.attention_relevance``),
        (B, gh, gw), detached.  One saving forward on a detached copy of the input that requires a gradient (so every
        block is differentiated) and one ``torch.autograd.grad`` of the summed score, during which the row vector
        ``r <- r + r A_l`` is propagated from the pooling head's map down through the blocks: one (B,N,N) buffer lives
        at a time.  No parameter's ``.grad`` and nothing of the caller's tensor is touched."""
        if not self.use_head:
            raise RuntimeError("attention_relevance reads the relevance through the pooling head's map and this model has "
                               "none; capture the block maps with capture_attention_gradients() and use "
                               "heads.attention_relevance(maps) for the (B,N,N) relevance")
        x = pixel_values.detach().clone().requires_grad_(True)
        state = {}

        def sink(layer, A):
            r = state.get("r", cap.pooling)
            if r is not None:
                state["r"] = r + torch.bmm(r.unsqueeze(1), A).squeeze(1)

        with torch.enable_grad(), self.capture_attention_gradients(heads="mean", kind="relevance", sink=sink) as cap:
            out = self(pixel_values=x, interpolate_pos_encoding=interpolate_pos_encoding)
            score = score_fn(out)
            torch.autograd.grad(score.sum(), x)
        if cap.pooling is None:
            raise RuntimeError("attention_relevance: score_fn did not depend on pooler_output, so the pooling head has no "
                               "map to read the relevance through; use capture_attention_gradients() and "
                               "heads.attention_relevance(maps) instead")
        r = state.get("r", cap.pooling)
        P = self.config.patch_size
        return r.detach().view(r.shape[0], x.shape[-2] // P, x.shape[-1] // P)

    def _run(self, pixel_values, output_hidden_states, interpolate_pos_encoding, hidden_state_ids, patches,
             keep_arena: bool = False):
        """The forward proper: (output, activation arena or None, (B, H, W)).  keep_arena (output_attentions): a call that
        would not train runs the saving forward all the same (no block keeps its GELU pre-activation: first = L), so the
        arena exists; a training call already has it."""
        layout, img_h, img_w = 0, 0, 0
        if patches is not None:
            if pixel_values is not None:
                raise ValueError("pass either pixel_values or patches")
            pixel_values, layout, img_h, img_w = patches.data, 2, int(patches.height), int(patches.width)
        if pixel_values.device.type != "cuda":
            raise RuntimeError("SiglipVisionModelHIP runs only on an AMD GPU through libsiglip_hip.so "
                               "(no CPU fallback); move the model and pixel_values to 'cuda'")
        # the input's own gradient (adversarial examples, saliency): the backward then runs through every block
        want_px = torch.is_grad_enabled() and pixel_values.requires_grad
        if want_px and layout == 2:
            raise RuntimeError("patches= with an operand that requires a gradient: the fused input transform "
                               "(preprocess.to_patch_operand) is not differentiable; pass the resized, normalised images "
                               "as pixel_values (B,3,H,W) with requires_grad=True instead, or detach the operand")
        if want_px and self.compute_dtype in INFERENCE_ONLY:
            raise RuntimeError(f"compute_dtype={self.compute_dtype!r} is inference-only and cannot differentiate with "
                               "respect to pixel_values: detach the input, or use compute_dtype='bf16' / 'fp16' / 'bf16x3' / "
                               "'fp32' for the gradient")
        L = self.config.num_hidden_layers
        if hidden_state_ids is not None:
            tap_ids = tuple(int(i) % (L + 1) for i in hidden_state_ids)
        elif output_hidden_states:
            tap_ids = tuple(range(L + 1))
        else:
            tap_ids = ()
        uniq = sorted(set(tap_ids))
        params = self._table.params()
        train = torch.is_grad_enabled() and (want_px or any(p.requires_grad for p in params))
        if train and self.compute_dtype in INFERENCE_ONLY:
            raise RuntimeError(f"compute_dtype={self.compute_dtype!r} is inference-only and cannot differentiate the "
                               "encoder: freeze it (encoder.requires_grad_(False); heads on top still train), run under "
                               "torch.no_grad(), or use compute_dtype='bf16' to train it")
        # first block that can receive a gradient (frozen prefix, Siglip2sidafrozen.py:757-768); 0 when the embeddings train
        # (an input that requires a gradient makes every block differentiable: first = 0)
        first = 0
        if train and not want_px and not any(p.requires_grad for p in params[:self._table.n_emb]):
            first = next((e.block for e, p in zip(self._table.entries, params) if p.requires_grad and e.block is not None),
                         L)
        save = train
        if keep_arena and not train:
            save, first = True, L
        outs = torch.ops.siglip_hip.encoder_fwd(pixel_values, params, self._handle, save,
                                                bool(interpolate_pos_encoding), self.use_head, uniq, first, layout, img_h,
                                                img_w, train and self._recompute)
        pooled = outs[0] if self.use_head else None
        hs = tuple(outs[2 + uniq.index(i)] for i in tap_ids) if tap_ids else None
        out = VisionModelOutput(last_hidden_state=outs[1], pooler_output=pooled, hidden_states=hs)
        if not keep_arena:
            return out, None, None
        return out, outs[-2], encoder_ops._input_geometry(self.config, pixel_values, layout, img_h, img_w)[:3]

    @torch.compiler.disable
    def forward_ragged(self, pixel_values, output_hidden_states: bool = False, hidden_state_ids=None):
        """Images of DIFFERENT sizes in one encoder call, without resizing and without padding (flash-attention "varlen"
        style).  ``pixel_values``: a sequence of normalised ``(3, H_i, W_i)`` or ``(1, 3, H_i, W_i)`` tensors on the GPU.
        The position table is always fitted to each image's grid (``interpolate_pos_encoding=True``).  Returns a
        ``RaggedVisionModelOutput`` (packed ``(T, D)`` token tensors, ``(S, D)`` ``pooler_output``); every value is
        bit-identical to ``model(pixel_values=x_i[None], interpolate_pos_encoding=True)`` of the image alone.

        Inference only.  It works under ``no_grad``, and with grad enabled when neither an input nor an encoder
        parameter requires a gradient (a head that trains on ``pooler_output`` of a frozen backbone); the outputs are
        outside autograd.  ``output_attentions``, ``patches=`` and the capture contexts are not offered here.  Not a custom
        op: under ``torch.compile`` the call is a graph break."""
        views, grids = encoder_ops.ragged_geometry(self.config, pixel_values)
        if torch.is_grad_enabled():
            one_per_size = ("forward_ragged is inference-only; to differentiate, make one call per image size: "
                            "model(pixel_values=batch_of_one_size, interpolate_pos_encoding=True)")
            if any(x.requires_grad for x in views):
                raise RuntimeError("forward_ragged: an input image requires a gradient. " + one_per_size)
            if any(p.requires_grad for p in self._table.params()):
                raise RuntimeError("forward_ragged: an encoder parameter requires a gradient (freeze the encoder with "
                                   "requires_grad_(False), or run under torch.no_grad()). " + one_per_size)
        if any(x.device.type != "cuda" for x in views):
            raise RuntimeError("SiglipVisionModelHIP runs only on an AMD GPU through libsiglip_hip.so "
                               "(no CPU fallback); move the model and every image to 'cuda'")
        L = self.config.num_hidden_layers
        if hidden_state_ids is not None:
            tap_ids = tuple(int(i) % (L + 1) for i in hidden_state_ids)
        elif output_hidden_states:
            tap_ids = tuple(range(L + 1))
        else:
            tap_ids = ()
        uniq = sorted(set(tap_ids))
        pooled, last, taps = encoder_ops.forward_ragged(self, views, grids, uniq)
        cu = [0]
        for gh, gw in grids:
            cu.append(cu[-1] + gh * gw)
        hs = tuple(taps[uniq.index(i)] for i in tap_ids) if tap_ids else None
        return RaggedVisionModelOutput(last_hidden_state=last, pooler_output=pooled, hidden_states=hs,
                                       grids=tuple(grids), cu_seqlens=tuple(cu))

    # ---- plumbing ----------------------------------------------------------------------------------------
    _RUNTIME = ("_table", "_contexts", "_shadows", "_grads", "_handle")

    def _new_runtime(self, reducer=None):
        """Everything that belongs to THIS Python object (not to its parameters): the state owners of ``encoder_state``
        and the op handle.  Never shared between two modules, never pickled."""
        self._table = ParamTable(self, self.config.num_hidden_layers, self.use_head)
        self._contexts = Contexts(self.config, self.compute_dtype, self.use_head)
        self._shadows = WeightShadows(self._table, self._contexts)
        self._grads = GradPlan(self._table)
        self._grads.set_reducer(reducer)
        self._handle = encoder_ops.register(self)

    def __copy__(self):
        """copy.copy: the same parameters and sub-modules behind fresh runtime state and a fresh op handle."""
        new = type(self).__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._new_runtime(self._grads.reducer)
        return new

    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in self._RUNTIME}

    def __setstate__(self, state):
        super().__setstate__(state)
        self._new_runtime()

    def __deepcopy__(self, memo):
        """copy.deepcopy (EMA / SWA wrappers): a fresh module with copied parameters and its own C context."""
        new = type(self)(self.config, self.compute_dtype, self.recompute)
        new.load_state_dict(self.state_dict())
        new.to(next(self.parameters()).device)
        for a, b in zip(new.parameters(), self.parameters()):
            a.requires_grad = b.requires_grad
        new.train(self.training)
        memo[id(self)] = new
        return new

    def set_grad_reducer(self, reducer) -> None:
        """Hand this module's gradient chunks to ``reducer`` (a ``ddp.GradBucketReducer``; its ``max_buckets`` sets the
        chunk plan) from the next backward on; None detaches.  Flat buffers cached for the previous plan are dropped."""
        self._grads.set_reducer(reducer)

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._shadows.invalidate(release=True)
        self._contexts.drop_workspace()
        self._grads.drop_buffers()
        return out


# ---------------------------------------------------------------------------------------------------------
# surface O
# ---------------------------------------------------------------------------------------------------------
class OpenClipStyleEncoder(nn.Module):
    """``open_clip`` image-tower surface: ``encode_image(x)`` returns the attention-pooled, un-normalised
    embedding (callers L2-normalise themselves: ``cifake_binary_classifier.py:728``)."""

    def __init__(self, config, compute_dtype: str = "bf16"):
        super().__init__()
        self.visual = SiglipVisionModelHIP(config, compute_dtype)
        self.embed_dim = self.visual.config.hidden_size
        self.image_size = self.visual.config.image_size
        # checkpoints keep open_clip's key names (``visual.trunk.blocks.N.attn.qkv.weight``): the reference saves and
        # reloads ``backbone.visual.trunk.*`` (cifake_binary_classifier.py:2089, train_fusion_head_only.py:110-122)
        self._register_state_dict_hook(self._timm_state_dict_hook)
        self._register_load_state_dict_pre_hook(self._timm_load_pre_hook, with_module=True)

    @staticmethod
    def _timm_state_dict_hook(module, state_dict, prefix, local_metadata):
        from . import weights_io
        pv = prefix + "visual.vision_model."
        hf = {k[len(pv):]: state_dict.pop(k) for k in [k for k in state_dict if k.startswith(pv)]}
        for k, v in weights_io.hf_to_timm(hf, module.visual.config, "trunk.").items():
            state_dict[prefix + "visual." + k] = v

    @staticmethod
    def _timm_load_pre_hook(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                            error_msgs):
        from . import weights_io
        pt = prefix + "visual.trunk."
        if any(k.startswith(pt) for k in state_dict):
            timm = {k[len(prefix + "visual."):]: state_dict[k] for k in state_dict if k.startswith(pt)}
            try:
                hf = weights_io.timm_to_hf(timm, module.visual.config, "trunk.")
            except (KeyError, ValueError) as e:   # incomplete / mis-shaped tower: report it the way torch reports keys
                error_msgs.append(f"open_clip vision tower under '{pt}' cannot be converted: {e!r}")
                return
            for k in list(timm):
                state_dict.pop(prefix + "visual." + k)
            for k, v in hf.items():
                state_dict[prefix + "visual." + k] = v
        for k in [k for k in state_dict if k.startswith(prefix + "text.") or k == prefix + "logit_scale"
                  or k == prefix + "logit_bias"]:
            state_dict.pop(k)  # the text tower is never used on this path (train_fusion_head_only.py:115)

    def named_parameters(self, prefix: str = "", recurse: bool = True, remove_duplicate: bool = True):
        """Parameter NAMES in open_clip/timm style (``visual.trunk.blocks.23.norm1.weight`` …): the reference selects what
        to unfreeze by substring (``'blocks.23'``, ``'norm'``, simple_classifier.py:489-493).  q/k/v stay separate tensors
        (``…attn.q_proj.weight``); the fused ``attn.qkv`` layout exists only in ``state_dict()``."""
        from . import weights_io
        root = prefix + ("." if prefix else "") + "visual."
        for name, p in super().named_parameters(prefix=prefix, recurse=recurse, remove_duplicate=remove_duplicate):
            if name.startswith(root):
                name = root + weights_io.hf_param_name_to_timm(name[len(root):])
            yield name, p

    def set_grad_checkpointing(self, enable: bool = True):
        """open_clip's name for gradient checkpointing: sets ``visual.recompute``."""
        self.visual.recompute = bool(enable)

    def encode_image(self, x=None, normalize: bool = False, patches=None):
        out = self.visual(pixel_values=x, interpolate_pos_encoding=False, patches=patches)
        f = out.pooler_output
        if normalize:
            f = f / f.norm(dim=-1, keepdim=True)
        return f

    def encode_image_ragged(self, images, normalize: bool = False):
        """``encode_image`` for a sequence of images of different sizes (``SiglipVisionModelHIP.forward_ragged``): (S, D),
        each row bit-identical to ``encode_image`` of that image with the position table fitted to its grid.  Inference
        only."""
        if not self.visual.use_head:
            raise RuntimeError("encode_image_ragged returns the pooling head's embedding and this model has no head")
        f = self.visual.forward_ragged(images).pooler_output
        if normalize:
            f = f / f.norm(dim=-1, keepdim=True)
        return f

    def forward(self, image):
        return self.encode_image(image)


def _preprocess_factory(image_size: int):
    """Resize(bilinear) + Normalize(0.5, 0.5) on an already-decoded float tensor in [0,1] (C,H,W)."""
    def preprocess(img: torch.Tensor) -> torch.Tensor:
        x = img.unsqueeze(0) if img.dim() == 3 else img
        if x.shape[-1] != image_size or x.shape[-2] != image_size:
            x = torch.nn.functional.interpolate(x, size=(image_size, image_size), mode="bilinear", align_corners=False)
        x = (x - 0.5) / 0.5
        return x[0] if img.dim() == 3 else x
    return preprocess


def create_model_and_transforms(model_name: str, pretrained: Optional[str] = None, device="cuda",
                                compute_dtype: str = "bf16", seed: int = 0):
    """Signature of ``open_clip.create_model_and_transforms`` as the reference calls it
    (``cifake_binary_classifier.py:625-629``).  ``pretrained`` may be a local checkpoint directory; the
    reference's ``'webli'`` tag needs the network, so it (like ``None``) selects seeded random init."""
    cfg = get_config(model_name)
    model = OpenClipStyleEncoder(cfg, compute_dtype)
    if pretrained and os.path.isdir(pretrained):
        from safetensors.torch import load_file
        model.visual.load_state_dict(vision_tower_only(load_file(os.path.join(pretrained, "model.safetensors"))))
    else:
        if pretrained:   # 'webli' & co.: a hub tag, not a local directory
            warnings.warn(f"create_model_and_transforms('{model_name}', pretrained='{pretrained}'): no network and no "
                          "local checkpoint directory — the encoder gets seeded RANDOM weights, not the pretrained "
                          "ones; pass pretrained=<dir with model.safetensors> for real weights", stacklevel=2)
        model.visual.load_state_dict(seeded_state_dict(cfg, seed))
    model = model.to(device)
    pre = _preprocess_factory(cfg.image_size)
    return model, pre, pre
