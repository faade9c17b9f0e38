"""Reference-owned heads, decoder and losses that sit on the encoder's outputs.

These are the small PyTorch modules the reference defines itself around the third-party ViT.  They consume the
HIP encoder's outputs through autograd; parameter names match the reference's modules so its checkpoints load
(`decoder.projs.N.proj.weight`, `cls_head.weight`, `se.0.weight`, `classifier.N.weight`, `mlp.0.weight`, …).
Parity is pinned by `tests/golden/heads_*.npz`, produced by `oracle/gen_golden_heads.py`, which executes the
reference's own class definitions (lifted from its source text in the build container) on seeded weights/inputs.

The decoder is the only piece with real HBM traffic; here the 1x1 `head` conv is applied BEFORE
the bilinear up-sampling — exact in real arithmetic because bilinear weights sum to one — so the
(B, E, img, img) tensor of the reference (151 MB per image at E=512, 384²) is never materialised.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .config import isqrt_exact
from . import lib as _lib
from .head_ops import (bce_dice_loss_from_lowres, combined_loss_from_lowres, depthwise3x3, gate_mul,
                       l2norm_temporal_mean, linear_tokens, seg_eval_from_lowres)


# ---------------------------------------------------------------------------------------------------------
# SID_Set multi-task model  (Siglip2sidafrozen.py:693-803)
# ---------------------------------------------------------------------------------------------------------
class _TapProj(nn.Module):
    """`LinearProj` (:693-696): keeps the `.proj` sub-module name of the reference checkpoints."""

    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.proj = nn.Linear(in_dim, out_dim)

    def forward(self, x):
        return linear_tokens(x, self.proj.weight, self.proj.bias)


class SegFormerMaskDecoder(nn.Module):
    """SegFormer-style mask decoder (`SegFormerStrongDecoder`, Siglip2sidafrozen.py:698-745).

    per tap: Linear(D→E) → (B,E,g,g) → depthwise 3x3 → 1x1 → GELU; concat K taps → channel gate
    (1x1 E·K→E·K/4 → GELU → 1x1 → sigmoid) ⊙ → 1x1 E·K→E → [1x1 E→1 ∘ bilinear up to target]."""

    def __init__(self, in_dims: Sequence[int], embed_dim: int = 256, dropout_rate: float = 0.0,
                 head_before_upsample: bool = True):
        super().__init__()
        k = len(in_dims)
        self.projs = nn.ModuleList([_TapProj(d, embed_dim) for d in in_dims])
        smooth = []
        for _ in in_dims:
            layers: List[nn.Module] = [nn.Conv2d(embed_dim, embed_dim, 3, padding=1, groups=embed_dim),
                                       nn.Conv2d(embed_dim, embed_dim, 1), nn.GELU()]
            if dropout_rate > 0:
                layers.append(nn.Dropout2d(p=dropout_rate))
            smooth.append(nn.Sequential(*layers))
        self.smooth = nn.ModuleList(smooth)
        self.fuse_attn = nn.Sequential(nn.Conv2d(embed_dim * k, (embed_dim * k) // 4, 1), nn.GELU(),
                                       nn.Conv2d((embed_dim * k) // 4, embed_dim * k, 1), nn.Sigmoid())
        fuse: List[nn.Module] = [nn.Conv2d(embed_dim * k, embed_dim, 1)]
        if dropout_rate > 0:
            fuse.append(nn.Dropout2d(p=dropout_rate))
        self.fuse = nn.Sequential(*fuse)
        self.head = nn.Conv2d(embed_dim, 1, 1)
        self.head_before_upsample = head_before_upsample

    @staticmethod
    def _pointwise(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
        """A 1x1 convolution on token-major data (..., C_in) -> (..., C_out): a plain GEMM instead of a MIOpen
        convolution; the parameters keep their Conv2d shapes, so checkpoints are unchanged."""
        return linear_tokens(x, conv.weight, conv.bias)

    def forward(self, hidden_list: Sequence[torch.Tensor], grid_hw: Tuple[int, int], target_size: int = 448,
                return_lowres: bool = False):
        """Everything up to the 1-channel logit map runs token-major / channels-last as GEMMs and elementwise ops (same
        math as the reference's NCHW convolutions, Siglip2sidafrozen.py:726-745); only the final bilinear up-sample of
        the (B,1,g,g) logits uses an NCHW tensor.  `return_lowres=True` stops before that up-sample and returns the
        (B,1,gh,gw) logits: `bce_dice_loss_from_lowres` consumes them without ever materialising (B,1,S,S)."""
        gh, gw = grid_hw
        feats = []
        for proj, smooth, h in zip(self.projs, self.smooth, hidden_list):
            x = proj(h)                                              # (B, N, E)
            b, _, e = x.shape
            x = depthwise3x3(x.reshape(b, gh, gw, e), smooth[0].weight, smooth[0].bias)
            x = F.gelu(self._pointwise(smooth[1], x))
            for extra in list(smooth)[3:]:                           # Dropout2d when configured: acts on channels
                x = extra(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
            feats.append(x)
        x = torch.cat(feats, dim=-1)                                 # (B, gh, gw, E*K)
        gate_pre = self._pointwise(self.fuse_attn[2], F.gelu(self._pointwise(self.fuse_attn[0], x)))
        x = self._pointwise(self.fuse[0], gate_mul(gate_pre, x))        # sigmoid(gate) * x in one pass on the GPU
        for extra in list(self.fuse)[1:]:
            x = extra(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        if self.head_before_upsample or return_lowres:
            logit = self._pointwise(self.head, x).permute(0, 3, 1, 2)   # (B, 1, gh, gw)
            if return_lowres:
                return logit
            return F.interpolate(logit, size=(target_size, target_size), mode="bilinear", align_corners=False)
        x = F.interpolate(x.permute(0, 3, 1, 2), size=(target_size, target_size), mode="bilinear", align_corners=False)
        return self.head(x)


class SigLIP2MTL(nn.Module):
    """3-class (real / synthetic / tampered) + mask-localisation model (`SigLIP2_MTL`,
    Siglip2sidafrozen.py:750-803) on the HIP encoder.  `forward(pixel_values) -> (cls_logit (B,3), seg_logits
    (B,1,S,S))`.  Only the taps the decoder needs are requested from the encoder."""

    def __init__(self, encoder: nn.Module, seg_layers: Sequence[int] = (2, 6, 10, -1), embed_dim: int = 256,
                 dropout_rate: float = 0.0, freeze_below: Optional[int] = None):
        super().__init__()
        self.encoder = encoder
        hid = encoder.config.hidden_size
        if freeze_below is not None:  # frozen variant (:754-768): embeddings + blocks < freeze_below
            for p in encoder.vision_model.embeddings.parameters():
                p.requires_grad = False
            for i, layer in enumerate(encoder.vision_model.encoder.layers):
                for p in layer.parameters():
                    p.requires_grad = i >= freeze_below
        self.cls_head = (nn.Sequential(nn.Dropout(p=dropout_rate), nn.Linear(hid, 3)) if dropout_rate > 0
                         else nn.Linear(hid, 3))
        self.seg_layers = tuple(seg_layers)
        self.decoder = SegFormerMaskDecoder([hid] * len(self.seg_layers), embed_dim=embed_dim,
                                            dropout_rate=dropout_rate)

    def forward(self, pixel_values, return_lowres: bool = False):
        """(cls_logit (B,3), seg_logits (B,1,S,S)) as the reference; `return_lowres=True` gives the (B,1,g,g) logit map
        instead (the training path of `training_loss`, which never forms the up-sampled logits)."""
        n_layers = self.encoder.config.num_hidden_layers
        idxs = [(i + 1 if i >= 0 else n_layers) for i in self.seg_layers]   # hs = [emb, h1..hL] (:790-793)
        out = self.encoder(pixel_values=pixel_values, hidden_state_ids=idxs, interpolate_pos_encoding=True)
        pooled = out.pooler_output if out.pooler_output is not None else out.last_hidden_state.mean(1)
        cls_logit = self.cls_head(pooled).squeeze(1)
        feats = list(out.hidden_states)
        g = isqrt_exact(feats[0].shape[1])
        seg_logits = self.decoder(feats, (g, g), target_size=int(pixel_values.shape[-1]), return_lowres=return_lowres)
        return cls_logit, seg_logits

    def training_loss(self, pixel_values, y_class, masks, has_mask, lam_seg: float = 1.0, bce_w: float = 1.0,
                      dice_w: float = 0.5, enhanced: bool = False, focal_w: float = 0.3, boundary_w: float = 0.4,
                      iou_w: float = 0.4, morph_w: float = 0.2):
        """The SID train-step loss (Siglip2sidafrozen.py:1375-1389: CE + lam * BCE/Dice on the samples with a mask) with the
        decoder tail fused for HBM: low-res logits -> loss directly.  ``bce_w`` / ``dice_w`` are the epoch-scheduled
        ``current_bce_w`` / ``current_dice_w`` the reference passes to ``bce_dice_loss`` (Siglip2sidafrozen.py:1340-1351,
        1389).  ``enhanced=True`` is the ``--use_enhanced_loss`` branch (:1379-1384): the segmentation term is
        ``combined_segmentation_loss`` with ``focal_w`` / ``boundary_w`` / ``morph_w`` = ``args.*`` and ``iou_w`` =
        ``current_iou_w`` (after the IoU-focused rescale of :1343-1351), again from the low-res logits
        (``combined_loss_from_lowres``); the four extra keywords are ignored otherwise.
        Returns (loss, cls_logit, seg_logits_lowres)."""
        cls_logit, seg_lr = self.forward(pixel_values, return_lowres=True)
        if enhanced:
            seg = combined_loss_from_lowres(seg_lr, masks, has_mask, bce_w=bce_w, focal_w=focal_w, dice_w=dice_w,
                                            boundary_w=boundary_w, iou_w=iou_w, morph_w=morph_w)
        else:
            seg = bce_dice_loss_from_lowres(seg_lr, masks, has_mask, bce_w=bce_w, dice_w=dice_w)
        loss = F.cross_entropy(cls_logit.float(), y_class) + lam_seg * seg
        return loss, cls_logit, seg_lr


# ---------------------------------------------------------------------------------------------------------
# binary heads on the pooled embedding
# ---------------------------------------------------------------------------------------------------------
def attention_rollout(attentions, residual: float = 0.5, pooling: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention rollout (Abnar & Zuidema 2020) of a ViT's per-block attention maps, e.g. the ``.attentions`` of
    ``SiglipVisionModelHIP(..., output_attentions=True)``, first block first.  Per block: the head mean A of a (B,H,N,N)
    tensor (a (B,N,N) one is taken as is), mixed with the residual path, ``(1 - residual) * A + residual * I``, rows
    renormalised; the rollout is the product of those matrices, last block leftmost: (B,N,N) in fp32.  With ``pooling``
    (the pooling head's probe attention, (B,H,N) or its head mean (B,N)) the result is ``pooling @ rollout``: (B,N), one
    relevance value per patch.  Plain torch (``bmm``)."""
    R = None
    for A in attentions:
        A = A.float()
        if A.dim() == 4:
            A = A.mean(1)
        eye = torch.eye(A.shape[-1], dtype=A.dtype, device=A.device)
        At = (1.0 - residual) * A + residual * eye
        At = At / At.sum(-1, keepdim=True)
        R = At if R is None else torch.bmm(At, R)
    if R is None:
        raise ValueError("attention_rollout needs at least one attention map")
    if pooling is None:
        return R
    p = pooling.float()
    if p.dim() == 3:
        p = p.mean(1)
    return torch.bmm(p.unsqueeze(1), R).squeeze(1)


def attention_relevance(maps, pooling: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient-weighted attention relevance (Chefer et al. 2021, "Generic Attention-model Explainability") from the
    per-block maps ``A_l = mean_h relu(P_l * dScore/dP_l)``, e.g. the ``.maps`` of
    ``SiglipVisionModelHIP.capture_attention_gradients(kind="relevance")``, first block first ((B,H,N,N) tensors are
    averaged over heads, (B,N,N) ones taken as is).  ``R <- R + A_l R`` from ``R = I``: the product of ``I + A_l``, last
    block leftmost, (B,N,N) in fp32.  With ``pooling`` (the pooling head's map, (B,H,N) or its head mean (B,N)) the
    result is the row ``pooling @ R``: (B,N), one relevance value per patch.  Plain torch (``bmm``)."""
    R = None
    for A in maps:
        A = A.float()
        if A.dim() == 4:
            A = A.mean(1)
        if R is None:
            R = A + torch.eye(A.shape[-1], dtype=A.dtype, device=A.device)
        else:
            R = R + torch.bmm(A, R)
    if R is None:
        raise ValueError("attention_relevance needs at least one map")
    if pooling is None:
        return R
    p = pooling.float()
    if p.dim() == 3:
        p = p.mean(1)
    return torch.bmm(p.unsqueeze(1), R).squeeze(1)


def l2_normalize(f: torch.Tensor, eps: float = 0.0) -> torch.Tensor:
    """`f / f.norm(dim=-1, keepdim=True)` (cifake_binary_classifier.py:728, hidf_video_classifier.py:308);
    eps=1e-6 is the `train_fusion_head_only.py:106` form."""
    return f / (f.norm(dim=-1, keepdim=True) + eps)


class SingleTokenAttention(nn.Module):
    """`LightweightAttention` (cifake_binary_classifier.py:574-595) applied to a length-1 sequence."""

    def __init__(self, dim: int, num_heads: int = 4):
        super().__init__()
        self.num_heads, self.head_dim = num_heads, dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        b, n, c = x.shape
        qkv = self.qkv(x).reshape(b, n, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * self.scale).softmax(dim=-1)
        return self.proj((attn @ qkv[2]).transpose(1, 2).reshape(b, n, c))


class CifakeBinaryHead(nn.Module):
    """Head of `FastBinaryClassifier` (cifake_binary_classifier.py:640-698,727-749): L2-norm → LayerNorm →
    (length-1 attention) → size-dependent MLP → scalar logit."""

    def __init__(self, feature_dim: int, model_size: str = "small", dropout_rate: float = 0.1,
                 use_lightweight_attention: bool = True):
        super().__init__()
        if use_lightweight_attention and model_size in ("tiny", "small"):
            self.attention: Optional[nn.Module] = SingleTokenAttention(feature_dim, num_heads=4)
        elif model_size == "large":
            self.attention = nn.MultiheadAttention(feature_dim, min(8, feature_dim // 64), dropout=dropout_rate,
                                                   batch_first=True)
        else:
            self.attention = None
        d = feature_dim
        if model_size == "tiny":
            self.classifier = nn.Sequential(nn.Dropout(dropout_rate * 0.5), nn.Linear(d, 1))
        elif model_size == "small":
            self.classifier = nn.Sequential(nn.Linear(d, d // 4), nn.GELU(), nn.Dropout(dropout_rate),
                                            nn.Linear(d // 4, 1))
        else:
            self.classifier = nn.Sequential(nn.Linear(d, d // 2), nn.GELU(), nn.Dropout(dropout_rate),
                                            nn.Linear(d // 2, d // 4), nn.GELU(), nn.Dropout(dropout_rate * 0.5),
                                            nn.Linear(d // 4, 1))
        self.layer_norm = nn.LayerNorm(d)

    def forward(self, features, return_features: bool = False):
        f = self.layer_norm(l2_normalize(features))
        if self.attention is not None:
            f = f.unsqueeze(1)
            f = self.attention(f) if isinstance(self.attention, SingleTokenAttention) else self.attention(f, f, f)[0]
            f = f.squeeze(1)
        return f if return_features else self.classifier(f).squeeze(-1)


class VideoBinaryHead(nn.Module):
    """Tail of `BinaryVideoClassifier` (hidf_video_classifier.py:276-320): per-frame L2-norm → mean over T →
    LayerNorm / MLP → one logit per clip.  Input: per-frame embeddings (B*T, D)."""

    def __init__(self, feature_dim: int, num_frames: int = 4, dropout_rate: float = 0.3):
        super().__init__()
        d = feature_dim
        self.num_frames = num_frames
        self.binary_classifier = nn.Sequential(
            nn.LayerNorm(d), nn.Dropout(dropout_rate), nn.Linear(d, d // 2), nn.ReLU(),
            nn.Dropout(dropout_rate * 0.67), nn.Linear(d // 2, d // 4), nn.ReLU(), nn.Dropout(dropout_rate * 0.33),
            nn.Linear(d // 4, 1))

    def forward(self, frame_features, batch_size: int):
        return self.binary_classifier(l2norm_temporal_mean(frame_features, batch_size)).squeeze(-1)


class SEBinaryHead(nn.Module):
    """SE gate + MLP of `BinaryClassifier` (train_fusion_head_only.py:84-109): f·σ(W2 relu(W1 f)) → MLP."""

    def __init__(self, dim: int = 1024):
        super().__init__()
        self.se = nn.Sequential(nn.Linear(dim, dim // 16), nn.ReLU(), nn.Linear(dim // 16, dim), nn.Sigmoid())
        self.classifier = nn.Sequential(nn.LayerNorm(dim), nn.Dropout(0.3), nn.Linear(dim, dim // 2), nn.GELU(),
                                        nn.Dropout(0.2), nn.Linear(dim // 2, dim // 4), nn.GELU(),
                                        nn.Linear(dim // 4, 1))

    def forward(self, pooled):
        f = l2_normalize(pooled, eps=1e-6)
        return self.classifier(f * self.se(f)).squeeze(-1)


class ImageBinaryHead(nn.Module):
    """Head of the HiDF image-track classifier (``BinaryClassifier.classifier`` + the L2-norm in front of it,
    simple_classifier.py:141-148,159-164): f/||f|| -> LayerNorm -> Dropout(0.3) -> Linear(D, D/2) -> GELU -> Dropout(0.2) ->
    Linear(D/2, 1) -> (B,).  Parameter names equal the reference's (``classifier.0.weight`` ...)."""

    def __init__(self, dim: int = 1024):
        super().__init__()
        self.classifier = nn.Sequential(nn.LayerNorm(dim), nn.Dropout(0.3), nn.Linear(dim, dim // 2), nn.GELU(),
                                        nn.Dropout(0.2), nn.Linear(dim // 2, 1))

    def forward(self, pooled):
        return self.classifier(l2_normalize(pooled)).squeeze(-1)


# ---------------------------------------------------------------------------------------------------------
# fusion / calibration  (train_fusion_head_only.py:230-317, appv3.py:1497-1510,1573-1578,3147-3182, coral.py:300-322)
# ---------------------------------------------------------------------------------------------------------
class TemperatureScaler(nn.Module):
    def __init__(self):
        super().__init__()
        self.T = nn.Parameter(torch.tensor(1.0))

    def forward(self, logits):
        return logits / (self.T + 1e-6)


class AdaptiveFusionHead(nn.Module):
    """w = softmax(MLP([zf, zs, |zf − zs|])); z = (w0·zf + w1·zs) / (T + 1e-6)."""

    def __init__(self, hidden_dim: int = 32):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(3, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, 2))
        self.temp = TemperatureScaler()

    def forward(self, z_freq, z_sig):
        w = F.softmax(self.mlp(torch.stack([z_freq, z_sig, (z_freq - z_sig).abs()], dim=-1)), dim=-1)
        return self.temp(w[..., 0] * z_freq + w[..., 1] * z_sig)


class LinearFusionHead(nn.Module):
    """The shipped 2→1 `FusionHead` (appv3.py:1573-1578; `siglip/fusion_head.safetensors`)."""

    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(2, 1)

    def forward(self, x):
        return self.fc(x)


class _FeatureNormalizer(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.register_buffer("mean", torch.zeros(dim))
        self.register_buffer("std", torch.ones(dim))

    def forward(self, x):
        return (x - self.mean) / (self.std + 1e-6)


class _ContrastScaler(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.alpha = nn.Parameter(torch.ones(dim))
        self.beta = nn.Parameter(torch.zeros(dim))

    def forward(self, x):
        return torch.tanh(self.alpha * x + self.beta)


class _BandGating(nn.Module):
    def __init__(self, dim, num_bands=4):
        super().__init__()
        assert dim % num_bands == 0
        self.band_dim, self.num_bands = dim // num_bands, num_bands
        self.gates = nn.Parameter(torch.zeros(num_bands))

    def forward(self, x):
        g = torch.sigmoid(self.gates).repeat_interleave(self.band_dim)
        return x * g


class _ResidualMLPBlock(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return x + self.fc2(F.gelu(self.fc1(self.norm(x))))


class FreqMLPv5(nn.Module):
    """v5 frequency-feature classifier (train_fusion_head_only.py:282-301)."""

    def __init__(self, dim: int = 24, hidden: int = 64, num_bands: int = 4):
        super().__init__()
        self.normer = _FeatureNormalizer(dim)
        self.contrast = _ContrastScaler(dim)
        self.band = _BandGating(dim, num_bands)
        self.blocks = nn.ModuleList([_ResidualMLPBlock(dim, hidden), _ResidualMLPBlock(dim, hidden)])
        self.head = nn.Linear(dim, 1)
        self.temp = TemperatureScaler()

    def forward(self, x):
        x = self.band(self.contrast(self.normer(x)))
        for blk in self.blocks:
            x = blk(x)
        return self.temp(self.head(x).squeeze(-1))


class _SafeLayerNorm(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))
        self.eps = eps

    def forward(self, x):
        mean = x.mean(dim=-1, keepdim=True)
        var = x.var(dim=-1, unbiased=False, keepdim=True)
        return (x - mean) / torch.sqrt(var + self.eps) * self.weight + self.bias


class FreqMLPApp(nn.Module):
    """The shipped app FreqMLP (appv3.py:1497-1510; `siglip/freq_mlp.safetensors`: net.0 LN(24), net.1 24→64,
    net.3 64→1).  The reference adds 0.001·randn jitter in eval mode (:1508-1509); `jitter=False` gives the
    deterministic function used for the known-answer test."""

    def __init__(self, in_dim: int = 24, hid: int = 64):
        super().__init__()
        self.net = nn.Sequential(_SafeLayerNorm(in_dim), nn.Linear(in_dim, hid), nn.GELU(), nn.Linear(hid, 1))

    def forward(self, x, jitter: bool = False):
        if jitter and not self.training:
            x = x + 0.001 * torch.randn_like(x)
        return self.net(x).squeeze(-1)


def _logit(p: float) -> float:
    p = min(max(p, 1e-6), 1 - 1e-6)
    return math.log(p / (1 - p))


class CoralCalibrator:
    """Ordinal 5-bin calibration (appv3.py:3154-3182): g_k = σ(z − c_k); p0 = 1−g0, p_k = g_{k−1}−g_k, p4 = g3."""

    def __init__(self, cutpoints: Optional[dict] = None, logit_cuts: Optional[Sequence[float]] = None):
        if logit_cuts is not None:
            cuts = list(logit_cuts)
        elif cutpoints:
            cuts = [_logit(cutpoints[k]) for k in ("q25", "q50", "q75", "max")]
        else:
            cuts = [_logit(0.32), _logit(0.47), _logit(0.61), _logit(0.75)]
        self.c = torch.tensor(cuts, dtype=torch.float32)

    @torch.no_grad()
    def probs(self, z_scaled):
        g = torch.sigmoid(torch.as_tensor(z_scaled, dtype=torch.float32) - self.c)
        p = torch.cat([1.0 - g[:1], g[:-1] - g[1:], g[-1:]])
        return p / (p.sum() + 1e-8)

    @torch.no_grad()
    def predict(self, z_scaled):
        p = self.probs(z_scaled)
        return int(torch.argmax(p).item()), p

    @torch.no_grad()
    def probs_batch(self, z_scaled: torch.Tensor) -> torch.Tensor:
        """Vectorised over a batch of fused logits (the app's 9-crop + rotated-view pattern, appv3.py:3221-3247)."""
        g = torch.sigmoid(z_scaled.float().unsqueeze(-1) - self.c.to(z_scaled.device))
        p = torch.cat([1.0 - g[..., :1], g[..., :-1] - g[..., 1:], g[..., -1:]], dim=-1)
        return p / (p.sum(dim=-1, keepdim=True) + 1e-8)


@torch.no_grad()
def app_freq_logits(images_u8: torch.Tensor, d, freq_mlp: nn.Module, jitter: bool = False):
    """``(z_freqs (1, C), z_freqs_cells (G, 1))``: the frequency-MLP logits `detect_core` computes per crop and
    `compute_patch_grid` per cell (appv3.py:3226-3237), in the shapes `core_signals_batched` takes for the image and for its
    cells.  ``d`` is `preprocess.detect_views(h, w)` of the one uint8 NHWC image ``images_u8``; one
    `preprocess.views_freq_features` pass over ``d.freq`` (the app's `extract_freq_vector` of every window) and one
    ``freq_mlp`` (`FreqMLPApp`) forward.  The app's eval-mode jitter is off unless ``jitter=True``."""
    from . import preprocess as _pp
    feats = _pp.views_freq_features(images_u8, [d.views[n] for n in d.freq])
    z = freq_mlp(feats, jitter=jitter)
    C = len(range(len(d.views))[d.crops])
    return z[:C][None], z[C:][:, None]


def app_visual_prob(z_views: torch.Tensor, d) -> torch.Tensor:
    """``(1,)``: the ``visual_prob`` of `core_signals_batched` (appv3.py:3231-3246) for the ``(V,)`` classifier logits of one
    image's view batch ``d = preprocess.detect_views(h, w)``: ``0.6 sigmoid(sum_c w_c z[d.crops]) + 0.4 sigmoid(z[d.rot])``,
    in plain differentiable torch (no ``no_grad``; fp32, or float64 for float64 logits).  With
    ``preprocess.views_resize_normalize(x, d.views, S, differentiable=True)`` as the encoder's ``pixel_values=`` it makes
    the app's visual probability a differentiable function of the source image ``x``.  The frequency branch reads integer
    SRM moments of a uint8 plane and has no gradient."""
    z = z_views if z_views.dtype == torch.float64 else z_views.float()
    w = d.weights.to(z.device, z.dtype)
    z_sig0 = (z[d.crops][None] * w).sum(-1)
    return 0.6 * torch.sigmoid(z_sig0) + 0.4 * torch.sigmoid(z[d.rot][None])


@torch.no_grad()
def core_signals_batched(z_sigs: torch.Tensor, crop_weights: torch.Tensor, z_freqs: torch.Tensor, z_rot: torch.Tensor,
                         fusion_head: nn.Module, coral: "CoralCalibrator", freq_temp: float = 1.25,
                         coral_temp: float = 1.0) -> dict:
    """The inference-side tail of the app's `detect_core` (appv3.py:3221-3300) for a BATCH of images, entirely on the
    device: weighted multi-crop logits, the 90-degree dual-view stabiliser, the 2->1 fusion head on probabilities, the
    temperature-scaled raw probability, the CORAL ordinal distribution with its Gaussian-smoothed probability and entropy,
    and the conservative blend.  The app does this per image with ~12 `.item()` round trips; here every quantity is a
    (B,) / (B,5) tensor and nothing synchronises.

    z_sigs, z_freqs: (B, C) per-crop logits of the SigLIP classifier and the frequency MLP (C = 9 crops,
    make_multicrops); crop_weights: (C,); z_rot: (B,) logit of the rotated view."""
    dev = z_sigs.device
    w = crop_weights.to(dev, torch.float32)
    z_sig0 = (z_sigs.float() * w).sum(-1)
    z_freq = (z_freqs.float() * w).sum(-1)
    visual_prob = 0.6 * torch.sigmoid(z_sig0) + 0.4 * torch.sigmoid(z_rot.float())
    pc = visual_prob.clamp(1e-6, 1 - 1e-6)
    z_sig = torch.log(pc / (1 - pc))                                     # _logit (appv3.py:3150-3152)
    p_freq = torch.sigmoid(z_freq / freq_temp)
    z = fusion_head(torch.stack([visual_prob, p_freq], dim=-1)).reshape(-1)
    z_scaled = z / max(float(coral_temp), 1e-3)
    p_fake_raw = torch.sigmoid(z_scaled)
    risk_probs = coral.probs_batch(z_scaled)                             # (B, 5)
    risk_idx = risk_probs.argmax(-1)
    risk_vec = torch.arange(5, dtype=torch.float32, device=dev)
    mu = (risk_probs * risk_vec).sum(-1)
    var = (risk_probs * (risk_vec - mu[:, None]) ** 2).sum(-1)
    p_coral = (mu / 4.0 + 0.5 * var).clamp(0.0, 1.0)
    entropy = -(risk_probs * torch.log(risk_probs + 1e-8)).sum(-1)
    p_blend = (0.70 * p_fake_raw + 0.30 * p_coral).clamp(0.0, 1.0)
    return {"z_sig": z_sig, "z_freq": z_freq, "visual_prob": visual_prob, "p_freq": p_freq, "z": z, "z_scaled": z_scaled,
            "p_fake_raw": p_fake_raw, "risk_probs": risk_probs, "risk_idx": risk_idx, "p_fake_coral": p_coral,
            "coral_entropy": entropy, "p_blend": p_blend}


RISK_NAMES = ["REAL", "LEAN_REAL", "BORDERLINE", "LEAN_FAKE", "FAKE"]


def fit_coral_cutpoints(logits: torch.Tensor, labels: torch.Tensor = None, num_classes: int = 5) -> List[float]:
    """15/35/55/75-percentile cut-points of the fused logits (coral.py:300-322: value at index int(q·n) of the
    ascending sort)."""
    s = np.sort(np.asarray(logits.detach().cpu().numpy() if torch.is_tensor(logits) else logits))
    return [float(s[int(q * len(s))]) for q in (0.15, 0.35, 0.55, 0.75)]


# ---------------------------------------------------------------------------------------------------------
# losses / metrics  (Siglip2sidafrozen.py:69-189, cifake_binary_classifier.py:238-251,788-792)
# ---------------------------------------------------------------------------------------------------------
def focal_loss(logits, targets, alpha: float = 0.25, gamma: float = 2.0):
    p = torch.sigmoid(logits)
    ce = F.binary_cross_entropy_with_logits(logits, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    alpha_t = alpha * targets + (1 - alpha) * (1 - targets)
    return (alpha_t * (1 - p_t) ** gamma * ce).mean()


def _box(x, k):
    return F.conv2d(x, torch.ones(1, 1, k, k, device=x.device, dtype=x.dtype), padding=k // 2)


def boundary_aware_loss(logits, targets, kernel_size: int = 3):
    """Convolution-morphology branch of the reference (Siglip2sidafrozen.py:107-115), the one taken when kornia
    is absent: boundary = dilate − erode by a k×k box; BCE weighted 1 + 3·boundary."""
    s = _box(targets, kernel_size)
    boundary = ((s > 0).float() - (s == kernel_size ** 2).float()).detach()
    bce = F.binary_cross_entropy_with_logits(logits, targets, reduction="none")
    return (bce * (1 + 3 * boundary)).mean()


def morphological_loss(logits, targets, kernel_size: int = 3):
    """Smoothness-penalty fallback branch (Siglip2sidafrozen.py:136-140)."""
    p = torch.sigmoid(logits)
    return (p[:, :, :, 1:] - p[:, :, :, :-1]).abs().mean() + (p[:, :, 1:, :] - p[:, :, :-1, :]).abs().mean()


def iou_loss(logits, targets, smooth: float = 1e-6):
    p = torch.sigmoid(logits)
    inter = (p * targets).sum(dim=(1, 2, 3))
    union = p.sum(dim=(1, 2, 3)) + targets.sum(dim=(1, 2, 3)) - inter + smooth
    return 1 - (inter / union).mean()


def _dice_term(logits, targets, eps):
    p = torch.sigmoid(logits)
    inter = (p * targets).sum(dim=(1, 2, 3))
    denom = p.sum(dim=(1, 2, 3)) + targets.sum(dim=(1, 2, 3)) + eps
    return 1 - (2 * inter / denom).mean()


def bce_dice_loss(logits, targets, bce_w: float = 1.0, dice_w: float = 0.5, eps: float = 1e-6):
    return bce_w * F.binary_cross_entropy_with_logits(logits, targets) + dice_w * _dice_term(logits, targets, eps)


def combined_segmentation_loss(logits, targets, bce_w=0.4, focal_w=0.3, dice_w=0.5, boundary_w=0.4, iou_w=0.4,
                               morph_w=0.2, eps=1e-6):
    return (bce_w * F.binary_cross_entropy_with_logits(logits, targets) + focal_w * focal_loss(logits, targets)
            + dice_w * _dice_term(logits, targets, eps) + boundary_w * boundary_aware_loss(logits, targets)
            + iou_w * iou_loss(logits, targets) + morph_w * morphological_loss(logits, targets))


def dice_iou_from_logits(logits, targets, thr: float = 0.5, eps: float = 1e-6):
    p_bin = (torch.sigmoid(logits) > thr).float()
    inter = (p_bin * targets).sum(dim=(1, 2, 3))
    union = (p_bin + targets - p_bin * targets).sum(dim=(1, 2, 3)) + eps
    dice = 2 * inter / (p_bin.sum(dim=(1, 2, 3)) + targets.sum(dim=(1, 2, 3)) + eps)
    return dice.detach().cpu().tolist(), (inter / union).detach().cpu().tolist(), p_bin


class MaskMetrics:
    """The localisation numbers of the SID validation loop (Siglip2sidafrozen.py:1424-1569) accumulated on the device from
    the LOW-RESOLUTION logits of `SigLIP2MTL.forward(..., return_lowres=True)`: Dice / IoU at `mask_thr`
    (`dice_iou_from_logits`, :183-189), the threshold sweep (`sweep_mask_thresholds`, :204-240) and the pixel AUC
    (`PixelAUCBuffer`, :1078-1106).  All three are functions of integer pixel counts that one HIP launch per batch produces
    (`head_ops.seg_eval_from_lowres`); `update` never synchronises with the host, `compute` does once.

    Cuts.  The reference predicts `sigmoid(z) > thr` on fp32 tensors; here a pixel is predicted when `z > logit(float32(thr))`
    (the logit formed in float64 and rounded to fp32).  The thresholds are `np.linspace(thr_min, thr_max, thr_steps)` plus
    `mask_thr`; they may come in any order and may repeat: the cuts are their sorted, de-duplicated logits and every
    threshold keeps the index of its cut, so the sweep still scans in the order given (ascending for the defaults).

    State (all additive, so `merge`, or `all_reduce(SUM)` on each tensor of `state()`, combines data-parallel ranks):
    `tp`, `fp`, `fn` int64 (K,) over all masked images; `dice_sum`, `iou_sum` float64 (K,), the sums over images of the
    per-image Dice / IoU; `count` int64 (3,) = masked images, foreground pixels, background pixels; `auc_hist` int64
    (2, 4096).

    Differences from the reference, all deliberate: the AUC is over ALL pixels (binned to 1/128 in logit, ties inside a bin
    counted one half; `pix_auc_halfwidth` bounds what the binning can hide) instead of a 400 000-pixel reservoir sample;
    soft masks are thresholded at 0.5 (SID masks are {0,1}); per-image ratios are formed in float64, not fp32.
    Out of scope: `--use_morphological_postprocess` (a Kornia opening on the full-resolution probabilities),
    `--early_exit_thresh` (a caller can zero the low-res rows of the skipped images: the bilinear map of zeros is zeros),
    overlays and plots."""

    STATE_KEYS = ("tp", "fp", "fn", "dice_sum", "iou_sum", "count", "auc_hist")

    def __init__(self, thr_min: float = 0.1, thr_max: float = 0.9, thr_steps: int = 17, mask_thr: float = 0.5,
                 eps: float = 1e-6):
        self.sweep_thresholds = np.linspace(thr_min, thr_max, thr_steps)
        self.mask_thr, self.eps = float(mask_thr), float(eps)
        thr = np.concatenate([self.sweep_thresholds, [self.mask_thr]])
        if not np.all((thr > 0) & (thr < 1)):
            raise ValueError("mask thresholds must lie strictly between 0 and 1")
        t32 = thr.astype(np.float32).astype(np.float64)
        logits = np.log(t32 / (1.0 - t32)).astype(np.float32)
        cuts, index = np.unique(logits, return_inverse=True)             # sorted, duplicates removed, thr -> cut
        if len(cuts) > 64:
            raise ValueError(f"{len(cuts)} distinct thresholds: sgl_op_seg_eval takes at most 64 cuts")
        self.cuts = cuts
        self.sweep_index, self.mask_index = index[:-1].astype(np.int64), int(index[-1])
        self._cuts_dev = {}          # device -> (pinned host copy, device copy)
        self._state = None

    # ---- state ---------------------------------------------------------------------------------------------------
    def _zeros(self, device):
        K, i64, f64 = len(self.cuts), torch.int64, torch.float64
        return {"tp": torch.zeros(K, dtype=i64, device=device), "fp": torch.zeros(K, dtype=i64, device=device),
                "fn": torch.zeros(K, dtype=i64, device=device), "dice_sum": torch.zeros(K, dtype=f64, device=device),
                "iou_sum": torch.zeros(K, dtype=f64, device=device), "count": torch.zeros(3, dtype=i64, device=device),
                "auc_hist": torch.zeros(2, _lib.SEG_EVAL_AUC_BINS, dtype=i64, device=device)}

    def _ensure(self, device):
        if self._state is None:
            self._state = self._zeros(device)
        elif self._state["tp"].device != torch.device(device):
            raise RuntimeError(f"MaskMetrics state lives on {self._state['tp'].device}, the update is on {device}")
        return self._state

    def reset(self):
        self._state = None

    def state(self) -> dict:
        """The accumulated tensors (on the device of the updates; zeros on the CPU before the first one)."""
        return dict(self._state if self._state is not None else self._zeros("cpu"))

    def load_state(self, state: dict):
        ref = self._zeros("cpu")
        for k in self.STATE_KEYS:
            if tuple(state[k].shape) != tuple(ref[k].shape) or state[k].dtype != ref[k].dtype:
                raise ValueError(f"state['{k}'] must be {ref[k].dtype} {tuple(ref[k].shape)}")
        self._state = {k: state[k].clone() for k in self.STATE_KEYS}
        return self

    def merge(self, other: "MaskMetrics"):
        """Add another accumulator's state (same thresholds) to this one."""
        if not np.array_equal(self.cuts, other.cuts) or not np.array_equal(self.sweep_index, other.sweep_index) \
                or self.mask_index != other.mask_index:
            raise ValueError("merge needs accumulators built with the same thresholds")
        if other._state is not None:
            mine = self._ensure(other._state["tp"].device if self._state is None else self._state["tp"].device)
            for k in self.STATE_KEYS:
                mine[k] += other._state[k].to(mine[k].device)
        return self

    # ---- accumulation ----------------------------------------------------------------------------------------------
    def device_cuts(self, device) -> torch.Tensor:
        """The fp32 cuts on `device`, uploaded once from pinned memory without blocking the host."""
        device = torch.device(device)
        if device not in self._cuts_dev:
            host = torch.from_numpy(self.cuts.copy())
            if device.type == "cuda":
                host = host.pin_memory()
            self._cuts_dev[device] = (host, host.to(device, non_blocking=True))
        return self._cuts_dev[device][1]

    @torch.no_grad()
    def update(self, logit_lr: torch.Tensor, masks: torch.Tensor, has_mask: torch.Tensor = None):
        """One validation batch: (B,1,g,g) low-res logits, (B,1,S,S) masks, (B,) has_mask.  One kernel launch and a few
        ops on (B, K+1) integers; nothing is copied to the host."""
        st = self._ensure(logit_lr.device)
        hist = seg_eval_from_lowres(logit_lr, masks, has_mask, cuts=self.device_cuts(logit_lr.device),
                                    auc_hist=st["auc_hist"])
        return self.update_from_hist(hist, has_mask)

    @torch.no_grad()
    def update_from_hist(self, hist: torch.Tensor, has_mask: torch.Tensor = None, auc_hist: torch.Tensor = None):
        """Accumulate from counts made elsewhere: `hist` (B, 2, K+1) as `seg_eval_from_lowres` returns it (any integer or
        float dtype, any device; rows of images outside `has_mask` are ignored), optionally a (2, 4096) `auc_hist` to add."""
        K = len(self.cuts)
        if hist.dim() != 3 or hist.shape[1] != 2 or hist.shape[2] != K + 1:
            raise ValueError(f"hist must be (B, 2, {K + 1}), got {tuple(hist.shape)}")
        st = self._ensure(hist.device)
        h = hist.to(torch.int64)
        if has_mask is not None:
            w = has_mask.to(device=h.device, dtype=torch.int64)
            h = h * w[:, None, None]
            n_img = w.sum()
        else:
            n_img = torch.full((), h.shape[0], dtype=torch.int64, device=h.device)
        above = h.flip(-1).cumsum(-1).flip(-1)          # above[b, c, k] = pixels of class c with at least k cuts below z
        tp, fp = above[:, 1, 1:], above[:, 0, 1:]       # predicted at cut j  <=>  k >= j + 1
        fg, bg = above[:, 1, 0], above[:, 0, 0]
        fn = fg[:, None] - tp
        tpf, pred, fgf = tp.double(), (tp + fp).double(), fg.double()[:, None]
        dice = 2.0 * tpf / (pred + fgf + self.eps)      # dice_iou_from_logits' eps placement, per image
        iou = tpf / ((pred + fgf - tpf) + self.eps)
        st["tp"] += tp.sum(0)
        st["fp"] += fp.sum(0)
        st["fn"] += fn.sum(0)
        st["dice_sum"] += dice.sum(0)                   # images outside has_mask contribute 0 / eps = 0
        st["iou_sum"] += iou.sum(0)
        st["count"] += torch.stack([n_img, fg.sum(), bg.sum()])
        if auc_hist is not None:
            st["auc_hist"] += auc_hist.to(device=h.device, dtype=torch.int64)
        return self

    # ---- results -----------------------------------------------------------------------------------------------------
    def compute(self) -> dict:
        """One device-to-host copy, then the reference's arithmetic on counts.  Keys: `dice`, `iou` (mean over masked images
        at `mask_thr`, 0.0 without any, as :1546-1547), `best` (the dict of `sweep_mask_thresholds`), `thresholds`,
        `f1_curve`, `dice_curve`, `iou_curve` (per sweep threshold), `pix_auc`, `pix_auc_halfwidth` (nan when a class has
        no pixel, as `PixelAUCBuffer.auc`), `num_images`."""
        st = self.state()
        K = len(self.cuts)
        packed = torch.cat([st["tp"], st["fp"], st["fn"], st["dice_sum"].view(torch.int64), st["iou_sum"].view(torch.int64),
                            st["count"], st["auc_hist"].reshape(-1)]).cpu()
        tp, fp, fn = (packed[i * K:(i + 1) * K].numpy() for i in range(3))
        dice_sum = packed[3 * K:4 * K].view(torch.float64).numpy()
        iou_sum = packed[4 * K:5 * K].view(torch.float64).numpy()
        n_img, n_fg, n_bg = (int(v) for v in packed[5 * K:5 * K + 3])
        auc_hist = packed[5 * K + 3:].reshape(2, -1).numpy()

        mean = (lambda s: s / n_img) if n_img else (lambda s: np.zeros_like(s))
        dice_c, iou_c = mean(dice_sum), mean(iou_sum)
        denom = 2.0 * tp + fp + fn
        f1_c = np.where(denom > 0, 2.0 * tp / np.maximum(denom, 1), 0.0)       # f1_score(..., zero_division=0)
        if n_fg == 0 or n_bg == 0:                                             # `len(np.unique(mask_flat)) > 1` fails
            f1_c = np.zeros_like(f1_c)
        best = {"f1": 0, "dice": 0, "iou": 0, "thr_f1": 0.5, "thr_dice": 0.5, "thr_iou": 0.5}
        curves = {"f1": [], "dice": [], "iou": []}
        for thr, j in zip(self.sweep_thresholds, self.sweep_index):
            vals = {"f1": float(f1_c[j]), "dice": float(dice_c[j]), "iou": float(iou_c[j])}
            for name, v in vals.items():
                curves[name].append(v)
                if n_img and v > best[name]:                                   # strict >, in scan order (:230-238)
                    best[name], best["thr_" + name] = v, float(thr)
        out = {"dice": float(dice_c[self.mask_index]), "iou": float(iou_c[self.mask_index]), "best": best,
               "thresholds": [float(t) for t in self.sweep_thresholds], "f1_curve": curves["f1"],
               "dice_curve": curves["dice"], "iou_curve": curves["iou"], "num_images": n_img}
        out["pix_auc"], out["pix_auc_halfwidth"] = self.auc_from_hist(auc_hist)
        return out

    @staticmethod
    def auc_from_hist(auc_hist) -> Tuple[float, float]:
        """(AUC, half-width) of a (2, NB) [background, foreground] histogram over increasing score bins: the probability that
        a foreground pixel's bin is above a background pixel's, pairs in the same bin counted one half; the half-width
        0.5 * sum_b pos_b neg_b / (P N) is the most the order inside the bins could add or take away."""
        neg, pos = np.asarray(auc_hist[0], dtype=np.float64), np.asarray(auc_hist[1], dtype=np.float64)
        P, N = pos.sum(), neg.sum()
        if P == 0 or N == 0:
            return float("nan"), float("nan")
        below = np.cumsum(neg) - neg
        same = float((pos * neg).sum())
        return float(((pos * below).sum() + 0.5 * same) / (P * N)), float(0.5 * same / (P * N))


class FocalLoss(nn.Module):
    """cifake_binary_classifier.py:238-251 (pt = exp(−bce) form)."""

    def __init__(self, alpha: float = 1.0, gamma: float = 2.0, pos_weight=None):
        super().__init__()
        self.alpha, self.gamma, self.pos_weight = alpha, gamma, pos_weight

    def forward(self, inputs, targets):
        bce = F.binary_cross_entropy_with_logits(inputs, targets, pos_weight=self.pos_weight, reduction="none")
        return (self.alpha * (1 - torch.exp(-bce)) ** self.gamma * bce).mean()


def label_smoothing_loss(pred, target, smoothing: float = 0.1):
    target = target.float() * (1 - smoothing) + 0.5 * smoothing
    return F.binary_cross_entropy_with_logits(pred, target)


def mtl_loss(cls_logit, seg_logits, y_class, masks, has_mask, lam_seg: float = 1.0, enhanced: bool = False):
    """Train-step loss of the SID script (Siglip2sidafrozen.py:1377-1389): CE + λ·seg-loss on the samples that
    carry a mask."""
    loss = F.cross_entropy(cls_logit, y_class)
    if has_mask.any():
        seg = combined_segmentation_loss if enhanced else bce_dice_loss
        loss = loss + lam_seg * seg(seg_logits[has_mask], masks[has_mask])
    return loss


# ---------------------------------------------------------------------------------------------------------
# composed task models (reference L3 modules: encoder surface O + head)
# ---------------------------------------------------------------------------------------------------------
class _FlatHeadKeys(nn.Module):
    """The reference's task models own their head layers directly (``se.0.weight``, ``classifier.5.bias`` …), ours
    keep them in ``self.head``; checkpoints use the reference's names, so the ``head.`` level is dropped on
    ``state_dict()`` and re-inserted on ``load_state_dict()`` (cifake_binary_classifier.py:2089,
    train_fusion_head_only.py:110-122)."""

    def __init__(self):
        super().__init__()
        self._register_state_dict_hook(self._flat_out)
        self._register_load_state_dict_pre_hook(self._flat_in, with_module=True)

    @staticmethod
    def _flat_out(module, state_dict, prefix, local_metadata):
        ph = prefix + "head."
        for k in [k for k in state_dict if k.startswith(ph)]:
            state_dict[prefix + k[len(ph):]] = state_dict.pop(k)

    @staticmethod
    def _flat_in(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        own = {n.split(".")[0] for n, _ in module.head.named_parameters()} | \
              {n.split(".")[0] for n, _ in module.head.named_buffers()}
        for k in [k for k in state_dict if k.startswith(prefix) and k[len(prefix):].split(".")[0] in own]:
            state_dict[prefix + "head." + k[len(prefix):]] = state_dict.pop(k)


class FastBinaryClassifierHIP(_FlatHeadKeys):
    """`FastBinaryClassifier.forward` (cifake_binary_classifier.py:714-749) on the HIP encoder: bilinear resize to
    the model resolution if needed → `backbone.encode_image` → head."""

    def __init__(self, backbone: nn.Module, model_size: str = "small", dropout_rate: float = 0.1,
                 use_lightweight_attention: bool = True):
        super().__init__()
        self.backbone = backbone
        self.resolution = backbone.image_size
        self.feature_dim = backbone.embed_dim
        self.head = CifakeBinaryHead(self.feature_dim, model_size, dropout_rate, use_lightweight_attention)

    def forward(self, x, return_features: bool = False):
        if x.shape[-1] != self.resolution:
            x = F.interpolate(x, size=(self.resolution, self.resolution), mode="bilinear", align_corners=False)
        return self.head(self.backbone.encode_image(x), return_features)


class BinaryVideoClassifierHIP(_FlatHeadKeys):
    """`BinaryVideoClassifier.forward` (hidf_video_classifier.py:299-320): (B,T,C,H,W) → per-frame encoder →
    L2-norm → temporal mean → MLP → (B,) logits."""

    def __init__(self, vision_encoder: nn.Module, num_frames: int = 4, dropout_rate: float = 0.3):
        super().__init__()
        self.vision_encoder = vision_encoder
        self.feature_dim = vision_encoder.embed_dim
        self.num_frames = num_frames
        self.head = VideoBinaryHead(self.feature_dim, num_frames, dropout_rate)

    def forward(self, x):
        b, t, c, h, w = x.shape
        return self.head(self.vision_encoder.encode_image(x.view(b * t, c, h, w)), batch_size=b)


class ImageBinaryClassifierHIP(_FlatHeadKeys):
    """`BinaryClassifier` of the HiDF image track (simple_classifier.py:115-164; BASELINE config 3 = this head on
    so400m-patch14-384): bilinear resize to the model resolution if needed -> `backbone.encode_image` -> L2-norm -> head
    -> (B,) logits.  ``partially_unfreeze_backbone()`` is the script's default fine-tuning recipe (:483-496)."""

    def __init__(self, backbone: nn.Module):
        super().__init__()
        self.backbone = backbone
        self.resolution = backbone.image_size
        self.feature_dim = backbone.embed_dim
        self.head = ImageBinaryHead(self.feature_dim)

    def forward(self, x):
        if x.shape[-1] != self.resolution:
            x = F.interpolate(x, size=(self.resolution, self.resolution), mode="bilinear")
        return self.head(self.backbone.encode_image(x))

    def partially_unfreeze_backbone(self, last_blocks: int = 2) -> int:
        """simple_classifier.py:483-496: freeze the whole backbone, then re-enable every parameter whose open_clip/timm
        NAME contains one of ``blocks.<L-1>`` ... ``blocks.<L-last_blocks>``, ``ln_final``, ``norm`` (the script
        hard-codes ``blocks.23`` / ``blocks.22`` for its 24-block tower).  Substring matching is kept as is: ``norm`` also
        selects ``norm1`` / ``norm2`` of EVERY block, the final norm and the pooling head's norm, and ``blocks.2`` style
        prefixes behave as in the script.  Returns the number of re-enabled parameters (what the script prints)."""
        for prm in self.backbone.parameters():
            prm.requires_grad = False
        depth = self.backbone.visual.config.num_hidden_layers
        keys = [f"blocks.{depth - 1 - i}" for i in range(last_blocks)] + ["ln_final", "norm"]
        n = 0
        for name, prm in self.backbone.named_parameters():
            if any(k in name for k in keys):
                prm.requires_grad = True
                n += prm.numel()
        return n


class SEBinaryClassifierHIP(_FlatHeadKeys):
    """`BinaryClassifier.forward` of the fusion script (train_fusion_head_only.py:101-109): frozen encoder under
    no_grad, nearest-neighbour resize to the model size, SE gate + MLP."""

    def __init__(self, backbone: nn.Module):
        super().__init__()
        self.backbone = backbone
        self.img_size = backbone.image_size
        self.head = SEBinaryHead(backbone.embed_dim)

    def forward(self, x):
        with torch.no_grad():
            if x.shape[-1] != self.img_size:
                x = F.interpolate(x, size=(self.img_size, self.img_size))
            f = self.backbone.encode_image(x)
        return self.head(f)
