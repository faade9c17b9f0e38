"""Generate tests/golden/attngrad/*.npz: the gradient of a score with respect to the attention probabilities of the REAL
``transformers.SiglipVisionModel``, and the gradient-weighted attention relevance composed from them.

Per case (the seeded weights and inputs of ``tests/gen_golden_attn.py``, whose files hold the probabilities themselves)
this runs the HF model (``attn_implementation="eager"``, fp32, CPU) with ``output_attentions=True`` under autograd, calls
``retain_grad()`` on every returned map, and differentiates

    score = sum_b pooler_output[b] . w,      w = randn(hidden_size) from torch.Generator().manual_seed(seed + 2000)

* ``<case>.l<i>.npz``  ``attn_grad``: ``attentions[i].grad``, (B,H,N,N) fp32, whole;
* ``<case>.npz``       ``score.w``; HF's OWN relative-L2 error on every layer's gradient under CPU bf16 / fp16 autocast
                       (``bf16ac.attn_grad.l2rel`` / ``fp16ac.*``, [L]: the yardsticks of the HIP 16-bit modes) and on the
                       relevance (``*.relevance.l2rel``); ``pooling_grad``: d score / d (pooling probabilities), (B,H,N);
                       ``relevance``: float64 (B,N), r = a_pool; r <- r + r A_l for l = L-1 .. 0 with
                       A_l = mean_h relu(P_l * dP_l), a_pool likewise from the pooling head.

``nn.MultiheadAttention`` returns a reshaped view of its weights, which receives no gradient, so the pooling head's
gradient comes from an explicit float64 restatement of the pooling attention (the head's own LayerNorm / MLP / out_proj
modules in float64 around a hand-written one-query softmax).  The restatement is first checked against HF: its pooled
output and its d score / d last_hidden_state (``restatement.pooled_err`` / ``.dlast_err``, relative, asserted <= 1e-5).

Data only; nothing outside tests/golden/attngrad is written.
Run once in a CPU container that has ``transformers``:  python tests/gen_golden_attn_grad.py [--only NAME]
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_attn as ga  # noqa: E402

gg = ga.gg
OUT_DIR = os.path.join(HERE, "golden", "attngrad")
NAMES = ("tiny_48", "tiny_208x176", "hostile_59x101")
CASES = [c for c in ga.CASES if c["name"] in NAMES]


def score_weight(D, seed):
    return torch.randn(D, generator=torch.Generator().manual_seed(seed + 2000))


def _grads(hf, x, w, dtype):
    """(attentions, their .grad, pooler_output, last_hidden_state, its .grad), fp32 or under CPU autocast(dtype)."""
    ctx = torch.autocast("cpu", dtype=dtype) if dtype is not None else torch.autocast("cpu", enabled=False)
    hf.zero_grad(set_to_none=True)
    with ctx:
        o = hf(pixel_values=x, output_attentions=True, interpolate_pos_encoding=True)
        for a in o.attentions:
            a.retain_grad()
        o.last_hidden_state.retain_grad()
        score = (o.pooler_output.float() @ w).sum()
    score.backward()
    assert all(a.grad is not None for a in o.attentions), "the returned maps are not in the graph"
    return ([a.detach().float() for a in o.attentions], [a.grad.float() for a in o.attentions],
            o.pooler_output.detach().float(), o.last_hidden_state.detach().float(), o.last_hidden_state.grad.float())


def pooling_restatement(hf, last, w, heads):
    """float64: (probabilities (B,H,N), their gradient, pooled, d score / d last)."""
    head = copy.deepcopy(getattr(hf, "vision_model", hf).head).double()
    h = last.double().clone().requires_grad_(True)
    B, N, D = h.shape
    dh = D // heads
    Wi, bi = head.attention.in_proj_weight, head.attention.in_proj_bias
    probe = head.probe.repeat(B, 1, 1)
    q = (probe @ Wi[:D].t() + bi[:D]).view(B, 1, heads, dh).transpose(1, 2)
    k = (h @ Wi[D:2 * D].t() + bi[D:2 * D]).view(B, N, heads, dh).transpose(1, 2)
    v = (h @ Wi[2 * D:].t() + bi[2 * D:]).view(B, N, heads, dh).transpose(1, 2)
    a = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, -1)          # (B,H,1,N)
    a.retain_grad()
    ao = (a @ v).transpose(1, 2).reshape(B, 1, D)
    h0 = head.attention.out_proj(ao)
    pooled = (h0 + head.mlp(head.layernorm(h0)))[:, 0]
    (pooled @ w.double()).sum().backward()
    return a.detach()[:, :, 0], a.grad[:, :, 0], pooled.detach(), h.grad


def relevance(att, grads, a_pool, g_pool):
    r = torch.relu(a_pool.double() * g_pool.double()).mean(1)
    for A, G in zip(reversed(att), reversed(grads)):
        Ab = torch.relu(A.double() * G.double()).mean(1)
        r = r + (r.unsqueeze(1) @ Ab).squeeze(1)
    return r


def _l2rel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def generate(case):
    config, weights = gg._light_package()
    cfg = config.get_config(case["config"])
    hf = ga._hf_model(cfg, weights.seeded_state_dict(cfg, seed=case["seed"]))
    H, W = gg.case_hw(case)
    x = weights.seeded_pixels(case["batch"], H, W, seed=case["seed"] + 1000)
    w = score_weight(cfg.hidden_size, case["seed"])
    att, grads, pooled, last, dlast = _grads(hf, x, w, None)
    a_pool, g_pool, pooled64, dlast64 = pooling_restatement(hf, last, w, cfg.num_attention_heads)
    pooled_err, dlast_err = _l2rel(pooled64, pooled), _l2rel(dlast64, dlast)
    assert pooled_err <= 1e-5 and dlast_err <= 1e-5, (pooled_err, dlast_err)
    rel = relevance(att, grads, a_pool, g_pool)
    L = len(att)
    rec = {"meta.config": np.asarray(case["config"]), "meta.seed": np.int64(case["seed"]),
           "meta.batch": np.int64(case["batch"]), "meta.res_h": np.int64(H), "meta.res_w": np.int64(W),
           "meta.layers": np.int64(L), "meta.transformers_version": np.asarray(__import__("transformers").__version__),
           "score.w": w.numpy(), "pooling_grad": g_pool.float().numpy(), "relevance": rel.numpy(),
           "restatement.pooled_err": np.float64(pooled_err), "restatement.dlast_err": np.float64(dlast_err)}
    for tag, dt in (("bf16ac.", torch.bfloat16), ("fp16ac.", torch.float16)):
        att_a, grads_a, _, last_a, _ = _grads(hf, x, w, dt)
        rec[tag + "attn_grad.l2rel"] = np.asarray([_l2rel(g, r) for g, r in zip(grads_a, grads)], dtype=np.float64)
        # the relevance HF's own autocast maps give, the pooling row from the restatement on ITS last_hidden_state
        ap, gp, _, _ = pooling_restatement(hf, last_a, w, cfg.num_attention_heads)
        rec[tag + "relevance.l2rel"] = np.float64(_l2rel(relevance(att_a, grads_a, ap, gp), rel))
    path = os.path.join(OUT_DIR, case["name"] + ".npz")
    np.savez_compressed(path, **rec)
    sizes = [os.path.getsize(path)]
    for i, g in enumerate(grads):
        p = os.path.join(OUT_DIR, f"{case['name']}.l{i}.npz")
        np.savez_compressed(p, attn_grad=g.numpy())
        sizes.append(os.path.getsize(p))
    print(f"wrote {path} + {L} layer files (largest {max(sizes) / 1024:.1f} KiB): grad shape {tuple(grads[0].shape)} "
          f"restatement {pooled_err:.1e} / {dlast_err:.1e}; l2rel bf16ac {rec['bf16ac.attn_grad.l2rel']} fp16ac "
          f"{rec['fp16ac.attn_grad.l2rel']}; relevance bf16ac {float(rec['bf16ac.relevance.l2rel']):.2e} fp16ac "
          f"{float(rec['fp16ac.relevance.l2rel']):.2e}", flush=True)


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    torch.set_num_threads(8)
    for c in gg.select_cases(CASES, sys.argv):
        generate(c)
