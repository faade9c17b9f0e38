"""The pixel-gradient fixtures (tests/golden/pixgrad/*.npz, written by tests/gen_golden_pixgrad.py from the real HF
SiglipVisionModel): case lists, loading, and the probe loss on device tensors.  A plain module: no tests, no fixtures."""
import os

import numpy as np
import torch

import golden_util as gu

DIR = os.path.join(gu.GOLDEN_DIR, "pixgrad")
EDGE_CASES = ["tiny_37x45_interp", "hostile_59x101_interp"]      # the patch size does not divide these
PREFIX_CASE = "tiny_48x37_prefix_taps"                             # shape, seed and taps of the frozen-prefix test
SMALL_CASES = gu.CASES + gu.RECT_CASES + EDGE_CASES + [PREFIX_CASE]
FULL_CASE = "so400m27_384"
CASES = SMALL_CASES + [FULL_CASE]
PREFIX = "grad.pixel_values"


def load(case):
    return dict(np.load(os.path.join(DIR, case + ".npz")))


def border_mask(B, H, W, P):
    """True on the trailing rows / columns no patch covers."""
    m = torch.zeros(B, 3, H, W, dtype=torch.bool)
    m[:, :, H // P * P:, :] = True
    m[:, :, :, W // P * P:] = True
    return m


def probe_loss(out, tap_ids):
    """oracle.probe_loss on tensors of any device."""
    def cw(t):
        idx = torch.arange(t.numel(), dtype=torch.float32, device=t.device).reshape(t.shape)
        return torch.cos(idx * 0.37 + 0.11)
    loss = (out.pooler_output * cw(out.pooler_output)).sum()
    loss = loss + 0.01 * (out.last_hidden_state * cw(out.last_hidden_state)).sum()
    for i in tap_ids:
        h = out.hidden_states[i]
        loss = loss + 0.01 * (h * cw(h)).sum()
    return loss


def ref_absmax(rec):
    return float(np.abs(rec[PREFIX + ".full"] if PREFIX + ".full" in rec else rec[PREFIX + ".samples"]).max())
