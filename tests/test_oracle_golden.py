"""CPU: the oracle restatement must reproduce the golden vectors captured from the real HF SiglipVisionModel
(forward outputs, every hidden-state tap, and gradients of the fixed probe loss)."""
import pytest
import torch

import golden_util as gu


@pytest.mark.parametrize("case", gu.CASES + gu.RECT_CASES)
def test_oracle_matches_hf_golden(case, pkg, oracle):
    rec = gu.load(case)
    m = gu.meta(rec)
    big = m["config"].startswith("so400m")
    cfg = pkg.get_config(m["config"])
    sd = pkg.weights.seeded_state_dict(cfg, seed=m["seed"])
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x = pkg.weights.seeded_pixels(m["batch"], m["res_h"], m["res_w"], seed=m["seed"] + 1000)
    torch.set_num_threads(8)
    out = oracle.vision_forward(x, sd, cfg, True, m["interp"])
    atol, rtol = (2e-5, 2e-5) if not big else (5e-5, 5e-5)
    gu.compare(rec, "pooler_output", out["pooler_output"].detach(), atol, rtol)
    gu.compare(rec, "last_hidden_state", out["last_hidden_state"].detach(), atol, rtol)
    assert len(out["hidden_states"]) == cfg.num_hidden_layers + 1
    for i, h in enumerate(out["hidden_states"]):
        gu.compare(rec, f"hidden_states.{i}", h.detach(), atol, rtol)
    loss = oracle.probe_loss(out, m["taps"])
    assert abs(loss.item() - float(rec["loss"])) <= 1e-3 * max(1.0, abs(float(rec["loss"])))
    loss.backward()
    checked = 0
    for k in rec:
        if k.startswith("grad.") and k.endswith(".shape"):
            name = k[len("grad."):-len(".shape")]
            gu.compare(rec, "grad." + name, sd[name].grad, 2e-4, 2e-4)
            checked += 1
    assert checked >= 20


def test_bicubic_table_matches_torch(oracle):
    """The explicit bicubic restatement equals F.interpolate(bicubic, align_corners=False)."""
    torch.manual_seed(0)
    for g0, gh, gw in [(2, 3, 3), (3, 7, 7), (14, 20, 20), (27, 16, 16), (27, 27, 27)]:
        t = torch.randn(g0 * g0, 24)
        ref = torch.nn.functional.interpolate(t.reshape(1, g0, g0, 24).permute(0, 3, 1, 2), size=(gh, gw),
                                              mode="bicubic", align_corners=False)
        ref = ref.permute(0, 2, 3, 1).reshape(gh * gw, 24)
        got = oracle.bicubic_resize_table(t, g0, gh, gw)
        assert (got - ref).abs().max().item() < 2e-5


def test_weight_generator_is_deterministic(pkg):
    cfg = pkg.get_config("tiny")
    a = pkg.weights.seeded_state_dict(cfg, 3)
    b = pkg.weights.seeded_state_dict(cfg, 3)
    c = pkg.weights.seeded_state_dict(cfg, 4)
    for k in a:
        assert torch.equal(a[k], b[k])
    assert not torch.equal(a["encoder.layers.0.mlp.fc1.weight"], c["encoder.layers.0.mlp.fc1.weight"])
    # known answer: pins the generator itself (splitmix64 + fnv1a), so fixtures stay valid
    v = pkg.weights.uniform_pm1("pixel_values", 4, seed=1234)
    assert v.dtype.name == "float32" and abs(float(v[0])) < 1.0
    assert pkg.weights.fnv1a64("a") == 0xAF63DC4C8601EC8C
