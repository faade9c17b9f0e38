"""Generate tests/golden/attn/*.npz: the attention maps of the REAL ``transformers.SiglipVisionModel``.

Per case this runs the HF model (``attn_implementation="eager"``, the seeded weights and input of ``oracle/gen_golden.py``)
in fp32 on the CPU with ``output_attentions=True`` and stores

* ``<case>.l<i>.npz``  ``attentions``: the (B,H,N,N) fp32 probabilities of block i, whole;
* ``<case>.npz``       ``pooling``: the pooling head's probe attention (B,H,N) (``nn.MultiheadAttention`` with
                       ``need_weights=True, average_attn_weights=False``), the meta data, and HF's OWN error on every
                       layer under CPU bf16 / fp16 autocast: ``bf16ac.attn.l2rel`` / ``.maxerr`` and ``fp16ac.*`` ([L] each,
                       plus ``*.pooling.l2rel`` / ``.maxerr``): the yardsticks of the HIP 16-bit modes.

One file per layer keeps every file far below the size limit of a committed file (the largest, 2x4x143x143 floats, is
0.65 MB before compression).  Data only; nothing outside tests/golden/attn is written.

Run once in a CPU container that has ``transformers``:  python tests/gen_golden_attn.py [--only NAME]
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT_DIR = os.path.join(HERE, "golden", "attn")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gg = _load("gen_golden", os.path.join(ROOT, "oracle", "gen_golden.py"))

CASES = [
    dict(name="tiny_48", config="tiny", seed=31, batch=2, res_h=48, res_w=48),            # N = 9: one partial tile
    dict(name="tiny_37x45", config="tiny", seed=32, batch=2, res_h=37, res_w=45),         # N = 4: edge rows ignored
    dict(name="tiny_208x176", config="tiny", seed=33, batch=2, res_h=208, res_w=176),     # N = 143 = 128 + 15
    dict(name="hostile_59x101", config="hostile", seed=34, batch=2, res_h=59, res_w=101),  # N = 28, head_dim 72 / DP 80
]


def _hf_model(cfg, sd):
    from transformers import SiglipVisionConfig as HFConfig, SiglipVisionModel
    hf = SiglipVisionModel(HFConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
        num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        image_size=cfg.image_size, patch_size=cfg.patch_size, attn_implementation="eager"))
    hf.load_state_dict(sd, strict=True)
    return hf.eval()


def _maps(hf, x, dtype):
    """(attentions tuple of (B,H,N,N), pooling (B,H,N)) in fp32 (dtype None) or under CPU autocast(dtype), as fp32."""
    ctx = torch.autocast("cpu", dtype=dtype) if dtype is not None else torch.autocast("cpu", enabled=False)
    with torch.no_grad(), ctx:
        o = hf(pixel_values=x, output_attentions=True, interpolate_pos_encoding=True)
        head = getattr(hf, "vision_model", hf).head   # transformers 5 dropped the vision_model level
        h = o.last_hidden_state
        probe = head.probe.repeat(h.shape[0], 1, 1)
        w = head.attention(probe, h, h, need_weights=True, average_attn_weights=False)[1]   # (B,H,1,N)
    return tuple(a.float() for a in o.attentions), w.float()[:, :, 0, :]


def _err(a, ref):
    d = (a.double() - ref.double())
    return float(d.norm() / ref.double().norm()), float(d.abs().max())


def generate(case):
    config, weights = gg._light_package()
    cfg = config.get_config(case["config"])
    hf = _hf_model(cfg, weights.seeded_state_dict(cfg, seed=case["seed"]))
    H, W = gg.case_hw(case)
    x = weights.seeded_pixels(case["batch"], H, W, seed=case["seed"] + 1000)
    att, pool = _maps(hf, x, None)
    L = len(att)
    rec = {"meta.config": np.asarray(case["config"]), "meta.seed": np.int64(case["seed"]),
           "meta.batch": np.int64(case["batch"]), "meta.res_h": np.int64(H), "meta.res_w": np.int64(W),
           "meta.layers": np.int64(L), "meta.transformers_version": np.asarray(__import__("transformers").__version__),
           "pooling": pool.numpy(),
           "rowsum.maxdev": np.float64(max(float((a.sum(-1) - 1).abs().max()) for a in att))}
    for tag, dt in (("bf16ac.", torch.bfloat16), ("fp16ac.", torch.float16)):
        att_a, pool_a = _maps(hf, x, dt)
        errs = [_err(a, r) for a, r in zip(att_a, att)]
        rec[tag + "attn.l2rel"] = np.asarray([e[0] for e in errs], dtype=np.float64)
        rec[tag + "attn.maxerr"] = np.asarray([e[1] for e in errs], dtype=np.float64)
        pe = _err(pool_a, pool)
        rec[tag + "pooling.l2rel"], rec[tag + "pooling.maxerr"] = np.float64(pe[0]), np.float64(pe[1])
    path = os.path.join(OUT_DIR, case["name"] + ".npz")
    np.savez_compressed(path, **rec)
    sizes = [os.path.getsize(path)]
    for i, a in enumerate(att):
        p = os.path.join(OUT_DIR, f"{case['name']}.l{i}.npz")
        np.savez_compressed(p, attentions=a.numpy())
        sizes.append(os.path.getsize(p))
    print(f"wrote {path} + {L} layer files (largest {max(sizes) / 1024:.1f} KiB): shape {tuple(att[0].shape)} rowsum dev "
          f"{float(rec['rowsum.maxdev']):.1e} l2rel bf16ac {rec['bf16ac.attn.l2rel']} fp16ac {rec['fp16ac.attn.l2rel']} "
          f"pooling bf16ac {float(rec['bf16ac.pooling.l2rel']):.2e}", flush=True)


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    torch.set_num_threads(8)
    for c in gg.select_cases(CASES, sys.argv):
        generate(c)
