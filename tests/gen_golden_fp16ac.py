"""Generate tests/golden/fp16ac/*.npz: the yardstick of the encoder's fp16 compute mode.

The reference's open_clip runs (cifake_binary_classifier.py, inference_*.py) use ``torch.amp.autocast('cuda')``, i.e.
float16.  For every case of ``oracle/gen_golden.py`` this runs the REAL ``transformers.SiglipVisionModel`` (same seeded
weights, input and probe loss) under ``torch.autocast("cpu", dtype=torch.float16)`` and stores its error against the fp32
values the existing fixture keeps, on exactly those elements, under ``fp16ac.<prefix>.maxerr`` / ``.l2rel`` (the
statistic gen_golden.py stores under ``bf16ac.*``).  The existing tests/golden/*.npz are read, never written.

It also writes ``so400m27_384.npz``: so400m-patch14-384, all 27 blocks, B=1, taps (13, 26), with HF fp32 samples of the
outputs, the taps and a handful of gradients, plus ``fp16ac.*`` and ``bf16ac.*`` statistics on them.

Run once in a CPU container that has ``transformers``:  python tests/gen_golden_fp16ac.py
``--only NAME`` writes one case only (and skips the full-depth file unless NAME is so400m27_384).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT_DIR = os.path.join(HERE, "golden", "fp16ac")


def _gen_golden():
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(ROOT, "oracle", "gen_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gg = _gen_golden()

FULL_CASE = dict(name="so400m27_384", config="so400m-patch14-384", seed=41, batch=1, res=384, interp=True, taps=(13, 26))
FULL_GRADS = ["embeddings.patch_embedding.weight",
              "encoder.layers.0.self_attn.q_proj.weight", "encoder.layers.0.mlp.fc1.weight",
              "encoder.layers.13.self_attn.q_proj.weight", "encoder.layers.13.mlp.fc1.weight",
              "encoder.layers.26.self_attn.q_proj.weight", "encoder.layers.26.mlp.fc1.weight",
              "post_layernorm.weight"]


def _hf_model(cfg, sd):
    from transformers import SiglipVisionConfig as HFConfig, SiglipVisionModel
    hf = SiglipVisionModel(HFConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
        num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        image_size=cfg.image_size, patch_size=cfg.patch_size, attn_implementation="eager"))
    hf.load_state_dict(sd, strict=True)
    hf.train()  # dropout is 0.0; the training path, as gen_golden.py
    return hf


def _run(hf, x, case, dtype):
    """forward + probe-loss backward, under CPU autocast(dtype) or in fp32 (dtype None); returns (tensors, loss)."""
    hf.zero_grad(set_to_none=True)
    ctx = torch.autocast("cpu", dtype=dtype) if dtype is not None else torch.autocast("cpu", enabled=False)
    with ctx:
        o = hf(pixel_values=x, output_hidden_states=True, interpolate_pos_encoding=case["interp"])
        out = {"pooler_output": o.pooler_output.float(), "last_hidden_state": o.last_hidden_state.float(),
               "hidden_states": tuple(h.float() for h in o.hidden_states)}
        loss = gg._oracle().probe_loss(out, case["taps"])
    loss.backward()
    t = {"pooler_output": out["pooler_output"], "last_hidden_state": out["last_hidden_state"]}
    for i, h in enumerate(out["hidden_states"]):
        t[f"hidden_states.{i}"] = h
    return t, loss.item()


def _errs(tag, rec, tensors, named, grads, out):
    """`tag`.<prefix>.maxerr / .l2rel against rec's fp32 values (gg.pack_err writes them as bf16ac.*)."""
    tmp = dict(rec)
    for prefix, t in tensors.items():
        if prefix + ".shape" in rec:
            gg.pack_err(prefix, t, tmp)
    for n in grads:
        if ("grad." + n + ".shape") in rec and named[n].grad is not None:
            gg.pack_err("grad." + n, named[n].grad, tmp)
    for k, v in tmp.items():
        if k.startswith("bf16ac.") and k not in ("bf16ac.loss",) and k.endswith((".maxerr", ".l2rel")):
            out[tag + k[len("bf16ac."):]] = v


def golden_cases():
    config, weights = gg._light_package()
    for case in gg.select_cases(gg.CASES + gg.RECT_CASES, sys.argv):
        rec = dict(np.load(os.path.join(ROOT, "tests", "golden", case["name"] + ".npz")))
        cfg = config.get_config(case["config"])
        hf = _hf_model(cfg, weights.seeded_state_dict(cfg, seed=case["seed"]))
        x = weights.seeded_pixels(case["batch"], *gg.case_hw(case), seed=case["seed"] + 1000)
        tensors, loss = _run(hf, x, case, torch.float16)
        out = {k: rec[k] for k in rec if k.startswith("meta.")}
        _errs("fp16ac.", rec, tensors, dict(hf.named_parameters()), gg.GRAD_NAMES, out)
        out["fp16ac.loss"] = np.float64(loss)
        path = os.path.join(OUT_DIR, case["name"] + ".npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}: pooled rel-L2 fp16ac {out['fp16ac.pooler_output.l2rel']:.2e} vs bf16ac "
              f"{float(rec['bf16ac.pooler_output.l2rel']):.2e}")


def full_depth():
    config, weights = gg._light_package()
    case = FULL_CASE
    cfg = config.get_config(case["config"])
    hf = _hf_model(cfg, weights.seeded_state_dict(cfg, seed=case["seed"]))
    x = weights.seeded_pixels(case["batch"], case["res"], case["res"], seed=case["seed"] + 1000)
    named = dict(hf.named_parameters())
    tensors, loss = _run(hf, x, case, None)
    rec = {"meta.config": np.asarray(case["config"]), "meta.seed": np.int64(case["seed"]),
           "meta.batch": np.int64(case["batch"]), "meta.res": np.int64(case["res"]),
           "meta.interp": np.int64(int(case["interp"])), "meta.taps": np.asarray(case["taps"], dtype=np.int64),
           "meta.transformers_version": np.asarray(__import__("transformers").__version__), "loss": np.float64(loss)}
    keep = ["pooler_output", "last_hidden_state"] + [f"hidden_states.{i}" for i in case["taps"]]
    for k in keep:
        gg.pack(k, tensors[k], rec)
    for n in FULL_GRADS:
        gg.pack("grad." + n, named[n].grad, rec)
    out = dict(rec)
    for tag, dt in (("fp16ac.", torch.float16), ("bf16ac.", torch.bfloat16)):
        t, l = _run(hf, x, case, dt)
        _errs(tag, rec, {k: t[k] for k in keep}, named, FULL_GRADS, out)
        out[tag + "loss"] = np.float64(l)
    path = os.path.join(OUT_DIR, case["name"] + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB): " + ", ".join(
        f"{k}: fp16ac {out['fp16ac.' + k + '.l2rel']:.2e} bf16ac {out['bf16ac.' + k + '.l2rel']:.2e}"
        for k in keep + ["grad." + n for n in FULL_GRADS]))


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    torch.set_num_threads(8)
    golden_cases()
    if "--no-full" not in sys.argv and gg.select_cases([FULL_CASE], sys.argv):
        full_depth()
