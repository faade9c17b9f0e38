"""Generate tests/golden/pixgrad/*.npz: d loss / d pixel_values of the REAL ``transformers.SiglipVisionModel``.

Per case this runs the HF model in fp32 on the CPU (the seeded weights, input and probe loss of ``oracle/gen_golden.py``),
with ``pixel_values.requires_grad_()``, and stores ``grad.pixel_values`` (``gg.pack``: full when small, strided samples +
checksums otherwise), then the error of the same model under CPU bf16 / fp16 autocast on exactly those elements
(``bf16ac.grad.pixel_values.maxerr`` / ``.l2rel`` and ``fp16ac.*``): the yardsticks of the HIP 16-bit modes.

Cases: every case of ``gen_golden.CASES`` and ``RECT_CASES``; two images the patch size does not divide (``EDGE_CASES``:
the trailing rows / columns feed nothing and carry a gradient of exactly 0, stored as ``border.absmax``); the case of the
frozen-prefix test (``PREFIX_CASE``); and the full-depth
``so400m27_384`` of ``tests/gen_golden_fp16ac.py``.  Nothing outside tests/golden/pixgrad is written.

Run once in a CPU container that has ``transformers``:  python tests/gen_golden_pixgrad.py [--only NAME]
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT_DIR = os.path.join(HERE, "golden", "pixgrad")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gg = _load("gen_golden", os.path.join(ROOT, "oracle", "gen_golden.py"))

# images the patch size does not divide: 37x45 at P = 16 (grid 2x2), 59x101 at P = 14 (grid 4x7)
EDGE_CASES = [
    dict(name="tiny_37x45_interp", config="tiny", seed=12, batch=2, res_h=37, res_w=45, interp=True, taps=(1, 3)),
    dict(name="hostile_59x101_interp", config="hostile", seed=13, batch=3, res_h=59, res_w=101, interp=True, taps=(0, 2)),
]
# the shape, seed and taps of the frozen-prefix test (tests/test_input_grad_gpu.py): the input gradient does not depend on
# which parameters are frozen, so HF's own run, and its error under autocast, is the yardstick of that configuration too
PREFIX_CASE = dict(name="tiny_48x37_prefix_taps", config="tiny", seed=21, batch=2, res_h=48, res_w=37, interp=True,
                   taps=(1, 2))
# the case of tests/golden/fp16ac/so400m27_384.npz (same seed, input and taps)
FULL_CASE = dict(name="so400m27_384", config="so400m-patch14-384", seed=41, batch=1, res=384, interp=True, taps=(13, 26))


def _hf_model(cfg, sd):
    from transformers import SiglipVisionConfig as HFConfig, SiglipVisionModel
    hf = SiglipVisionModel(HFConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
        num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        image_size=cfg.image_size, patch_size=cfg.patch_size, attn_implementation="eager"))
    hf.load_state_dict(sd, strict=True)
    hf.train()  # dropout is 0.0; the training path, as gen_golden.py
    for p in hf.parameters():
        p.requires_grad_(False)   # the gradient asked for is the input's
    return hf


def _pixel_grad(hf, x, case, dtype):
    """d probe_loss / d pixel_values in fp32 (dtype None) or under CPU autocast(dtype)."""
    x = x.clone().requires_grad_(True)
    ctx = torch.autocast("cpu", dtype=dtype) if dtype is not None else torch.autocast("cpu", enabled=False)
    with ctx:
        o = hf(pixel_values=x, output_hidden_states=True, interpolate_pos_encoding=case["interp"])
        out = {"pooler_output": o.pooler_output.float(), "last_hidden_state": o.last_hidden_state.float(),
               "hidden_states": tuple(h.float() for h in o.hidden_states)}
        loss = gg._oracle().probe_loss(out, case["taps"])
    loss.backward()
    return x.grad.detach().float(), loss.item()


def generate(case):
    config, weights = gg._light_package()
    cfg = config.get_config(case["config"])
    hf = _hf_model(cfg, weights.seeded_state_dict(cfg, seed=case["seed"]))
    H, W = gg.case_hw(case)
    x = weights.seeded_pixels(case["batch"], H, W, seed=case["seed"] + 1000)
    g, loss = _pixel_grad(hf, x, case, None)
    rec = {"meta.config": np.asarray(case["config"]), "meta.seed": np.int64(case["seed"]),
           "meta.batch": np.int64(case["batch"]), "meta.res_h": np.int64(H), "meta.res_w": np.int64(W),
           "meta.interp": np.int64(int(case["interp"])), "meta.taps": np.asarray(case["taps"], dtype=np.int64),
           "meta.transformers_version": np.asarray(__import__("transformers").__version__), "loss": np.float64(loss)}
    gg.pack("grad.pixel_values", g, rec)
    P = cfg.patch_size
    border = torch.cat([g[:, :, H // P * P:, :].reshape(-1), g[:, :, :, W // P * P:].reshape(-1)])
    rec["border.absmax"] = np.float64(border.abs().max().item() if border.numel() else 0.0)
    for tag, dt in (("bf16ac.", torch.bfloat16), ("fp16ac.", torch.float16)):
        ga, la = _pixel_grad(hf, x, case, dt)
        tmp = dict(rec)
        gg.pack_err("grad.pixel_values", ga, tmp)   # writes bf16ac.grad.pixel_values.*
        rec[tag + "grad.pixel_values.maxerr"] = tmp["bf16ac.grad.pixel_values.maxerr"]
        rec[tag + "grad.pixel_values.l2rel"] = tmp["bf16ac.grad.pixel_values.l2rel"]
        rec[tag + "loss"] = np.float64(la)
    path = os.path.join(OUT_DIR, case["name"] + ".npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB): max|g| {g.abs().max().item():.3e} border "
          f"{float(rec['border.absmax']):.1e} l2rel bf16ac {float(rec['bf16ac.grad.pixel_values.l2rel']):.2e} fp16ac "
          f"{float(rec['fp16ac.grad.pixel_values.l2rel']):.2e}", flush=True)


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    torch.set_num_threads(8)
    for c in gg.select_cases(gg.CASES + gg.RECT_CASES + EDGE_CASES + [PREFIX_CASE, FULL_CASE], sys.argv):
        generate(c)
