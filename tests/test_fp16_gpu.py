"""GPU tests of the fp16 compute mode (fp16 MFMA operands, fp32 accumulate / residual stream / statistics / softmax).

The reference's open_clip runs train and evaluate under ``torch.amp.autocast('cuda')`` (float16) with a ``GradScaler``
(cifake_binary_classifier.py:824-841,915,1948; inference_ai_human_images.py:279).  The yardstick is therefore the error
the REAL HF model makes under fp16 autocast against its own fp32 run: ``fp16ac.*`` in tests/golden/fp16ac/*.npz
(tests/gen_golden_fp16ac.py).  Bars:

  * ops: fp16 kernels vs an fp32 computation on the SAME fp16 operands, so the only differences are the accumulation order
    and the rounding of fp16 outputs (2^-11 relative) / of the P and dS operands inside attention;
  * encoder, every golden case and full-depth so400m@384: rel-L2 <= 2x and max-err <= 3x HF-fp16-autocast's, and the
    fp16 mode must be clearly more accurate than the bf16 mode on the same inputs (it really runs fp16 arithmetic);
  * a cifake-style autocast + GradScaler training loop against fp32 CPU AdamW, including an overflowing step that the
    scaler must skip without touching anything.
"""
import math
import os

import numpy as np
import pytest
import torch

import golden_util as gu
from attn_util import attn_reference, run_attention

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 3
FP16_DIR = os.path.join(gu.GOLDEN_DIR, "fp16ac")


@pytest.fixture(scope="module")
def lib(hiplib):
    assert torch.cuda.is_available()
    return hiplib


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def ok(st):
    assert st == 0, f"C ABI status {st}"


def relerr(got, ref):
    got, ref = got.float(), ref.float()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


def gelu_tanh(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


def call_gemm_nt(lib, dtype, A, B, M, N, K, epi, out, ldo, out2=None, ldo2=0, bias=None, res=None, ldr=0, aux=None,
                 ldaux=0, pos=None, pos_rows=1, tokens=1, heads=1, hd=8, hdp=8, batch=1):
    return lib.sgl_op_gemm_nt(dtype, P(A), A.stride(0), P(B), B.stride(0), M, N, K, epi, P(out), ldo, P(out2), ldo2,
                              P(bias), P(res), ldr, P(aux), ldaux, P(pos), pos_rows, tokens, heads, hd, hdp, batch,
                              stream())


# fp16 output: 2^-11 relative rounding of each element (relerr is relative to the tensor's max, so ~half of that),
# fp32 output: accumulation order only
TOL_F16_OUT, TOL_F32_OUT = 1.5e-3, 3e-5

# ---------------------------------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------------------------------
# M = 93 312 is the so400m@384 token count at B = 128; reduced-M shapes cover every (N, K) of the encoder and the tails,
# small ones the 128x128-tile kernel
NT_SHAPES = [(93312, 1152, 1152), (2916, 3456, 1152), (2916, 4352, 1152), (2916, 1152, 4352), (2300, 4352, 1152),
             (2051, 1160, 200), (729, 1152, 1152), (300, 1152, 4352), (64, 4352, 1152), (200, 136, 72), (1, 8, 8)]


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_f16_store(lib, M, N, K):
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device="cuda").half()
    B = (torch.randn(N, K, device="cuda") / math.sqrt(K)).half()
    bias = torch.randn(N, device="cuda")
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float16)
    ok(call_gemm_nt(lib, F16, A, B, M, N, K, 0, out, N, bias=bias))
    ref = torch.addmm(bias, A.float(), B.float().t())
    assert relerr(out, ref) < TOL_F16_OUT
    o32 = torch.empty(M, N, device="cuda")
    ok(call_gemm_nt(lib, F16, A, B, M, N, K, 6, o32, N, bias=bias))
    assert relerr(o32, ref) < TOL_F32_OUT


@pytest.mark.parametrize("M", [333, 2333, 5832])
def test_gemm_nt_f16_epilogues(lib, M):
    torch.manual_seed(M)
    N, K = 384, 192
    A = torch.randn(M, K, device="cuda").half()
    B = (torch.randn(N, K, device="cuda") / math.sqrt(K)).half()
    bias = torch.randn(N, device="cuda")
    acc = A.float() @ B.float().t()
    u = torch.empty(M, N, device="cuda", dtype=torch.float16)
    a = torch.empty(M, N, device="cuda", dtype=torch.float16)
    ok(call_gemm_nt(lib, F16, A, B, M, N, K, 1, u, N, out2=a, ldo2=N, bias=bias))
    assert relerr(u, acc + bias) < TOL_F16_OUT
    assert relerr(a, gelu_tanh(acc + bias)) < TOL_F16_OUT
    res = torch.randn(M, N, device="cuda")
    o = torch.empty(M, N, device="cuda")
    ok(call_gemm_nt(lib, F16, A, B, M, N, K, 2, o, N, bias=bias, res=res, ldr=N))
    assert relerr(o, res + acc + bias) < TOL_F32_OUT
    uu = (torch.randn(M, N, device="cuda") * 1.5).half()
    o2 = torch.empty(M, N, device="cuda", dtype=torch.float16)
    ok(call_gemm_nt(lib, F16, A, B, M, N, K, 4, o2, N, aux=uu, ldaux=N))
    ur = uu.float().requires_grad_(True)
    gelu_tanh(ur).backward(acc)
    assert relerr(o2, ur.grad) < TOL_F16_OUT
    pos = torch.randn(37, N, device="cuda")
    o3 = torch.empty(M, N, device="cuda")
    ok(call_gemm_nt(lib, F16, A, B, M, N, K, 5, o3, N, bias=bias, pos=pos, pos_rows=37))
    assert relerr(o3, acc + bias + pos[torch.arange(M, device="cuda") % 37]) < TOL_F32_OUT


@pytest.mark.parametrize("batch,tokens,heads,hd", [(2, 9, 2, 72), (3, 729, 16, 72), (11, 196, 12, 64)])
def test_gemm_nt_f16_qkv_scatter(lib, batch, tokens, heads, hd):
    torch.manual_seed(11)
    D = heads * hd
    hdp = (hd + 15) // 16 * 16
    M, N, K = batch * tokens, 3 * D, D
    A = torch.randn(M, K, device="cuda").half()
    B = (torch.randn(N, K, device="cuda") / math.sqrt(K)).half()
    bias = torch.randn(N, device="cuda")
    out = torch.full((3, batch, heads, tokens, hdp), float("nan"), device="cuda", dtype=torch.float16)
    ok(call_gemm_nt(lib, F16, A, B, M, N, K, 3, out, 0, bias=bias, tokens=tokens, heads=heads, hd=hd, hdp=hdp,
                    batch=batch))
    ref = (A.float() @ B.float().t() + bias).view(batch, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4)
    assert relerr(out[..., :hd], ref) < TOL_F16_OUT
    if hdp > hd:
        assert (out[..., hd:] == 0).all()


def test_gemm_nt_f16_overflow_is_inf_not_clamped(lib):
    """Outputs past fp16's range become +-inf (what GradScaler's found-inf check needs), never a saturated 65504."""
    M, N, K = 2304, 256, 64
    A = torch.full((M, K), 300.0, device="cuda", dtype=torch.float16)
    A[1::2] = -300.0
    B = torch.full((N, K), 300.0, device="cuda", dtype=torch.float16)
    for m in (M, 200):   # 256x256-tile and 128x128-tile kernels
        out = torch.zeros(m, N, device="cuda", dtype=torch.float16)
        ok(call_gemm_nt(lib, F16, A[:m], B, m, N, K, 0, out, N))
        assert torch.isinf(out).all()
        assert (out[0::2] > 0).all() and (out[1::2] < 0).all()


@pytest.mark.parametrize("Mred,N1,N2", [(93312 // 8, 1152, 1152), (2916, 1152, 4352), (5000, 4352, 1152),
                                        (4100, 3456, 1152), (2916, 1152, 3456), (729, 144, 144), (2187, 538, 144),
                                        (130, 8, 16)])
def test_gemm_tn_ws_f16(lib, Mred, N1, N2):
    torch.manual_seed(Mred + N1)
    lda, ldb = (N1 + 7) // 8 * 8 + 8, (N2 + 7) // 8 * 8
    A = torch.zeros(Mred, lda, device="cuda", dtype=torch.float16)
    B = torch.zeros(Mred, ldb, device="cuda", dtype=torch.float16)
    A[:, :N1] = torch.randn(Mred, N1, device="cuda").half()
    B[:, :N2] = torch.randn(Mred, N2, device="cuda").half()
    ref = A[:, :N1].float().t() @ B[:, :N2].float()
    scratch = torch.empty(64 << 18, device="cuda")   # 64 MiB: always enough for the deterministic split-K form
    outs = []
    for _ in range(2):
        out = torch.full((N1, N2), float("nan"), device="cuda")
        ok(lib.sgl_op_gemm_tn_ws(F16, P(A), lda, P(B), ldb, Mred, N1, N2, 0, P(out), N2, 0, P(scratch),
                                 scratch.numel() * 4, stream()))
        outs.append(out)
    assert relerr(outs[0], ref) < TOL_F32_OUT
    assert torch.equal(outs[0], outs[1]), "split-K with scratch must be bitwise reproducible"
    ok(lib.sgl_op_gemm_tn_ws(F16, P(A), lda, P(B), ldb, Mred, N1, N2, 0, P(outs[0]), N2, 1, P(scratch),
                             scratch.numel() * 4, stream()))
    assert relerr(outs[0], 2 * ref) < TOL_F32_OUT


def attention_errors(lib, dtype, qkv, dout_tok, B, H, N, dh, layout):
    """relerr of O, dQ, dK, dV and the largest |lse| error against fp32 eager + autograd on the same rounded inputs."""
    tdt = {BF16: torch.bfloat16, F16: torch.float16}[dtype]
    q, k, v = qkv.to(tdt)
    dout = dout_tok.to(tdt).view(B, N, H, dh).permute(0, 2, 1, 3)
    out, lse, dq, dk, dv = run_attention(lib, dtype, layout, q, k, v, dout)
    ref = attn_reference(q, k, v, dout)
    return dict(out=relerr(out, ref[0]), lse=(lse - ref[1]).abs().max().item(), dq=relerr(dq, ref[2]),
                dk=relerr(dk, ref[3]), dv=relerr(dv, ref[4]))


@pytest.mark.parametrize("B,H,N,dh", [(2, 16, 729, 72), (1, 12, 196, 64), (2, 2, 9, 72), (1, 2, 130, 32)])
@pytest.mark.parametrize("layout", ["token", "head"])
def test_attention_f16_fwd_bwd(lib, B, H, N, dh, layout):
    """fp16 flash attention vs fp32 eager + autograd on the same fp16 inputs.  The fp16 kernels round P and dS to fp16
    (2^-11) where the bf16 ones round to 2^-8: the errors must be several times smaller than bf16's on the same data."""
    torch.manual_seed(N + dh)
    qkv = torch.randn(3, B, H, N, dh, device="cuda") * 1.2
    dout = torch.randn(B * N, H * dh, device="cuda")
    e16 = attention_errors(lib, F16, qkv, dout, B, H, N, dh, layout)
    eb = attention_errors(lib, BF16, qkv, dout, B, H, N, dh, layout)
    print(f"[attn fp16 {B},{H},{N},{dh} {layout}] " + ", ".join(f"{k} {e16[k]:.2e} (bf16 {eb[k]:.2e})" for k in e16))
    assert e16["out"] < 3e-3 and e16["lse"] < 2e-3
    for k in ("dq", "dk", "dv"):
        assert e16[k] < 6e-3, (k, e16[k])
    for k in ("out", "dq", "dk", "dv"):
        assert e16[k] <= 0.5 * eb[k] + 1e-4, (k, e16[k], eb[k])


# ---------------------------------------------------------------------------------------------------------------------
# encoder parity against HF under fp16 autocast
# ---------------------------------------------------------------------------------------------------------------------
def _build(pkg, cfg, seed, mode):
    model = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode)
    model.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=seed))
    return model.to("cuda")


def _probe_loss(out, tap_ids):
    def cw(t):
        idx = torch.arange(t.numel(), dtype=torch.float32, device=t.device).reshape(t.shape)
        return torch.cos(idx * 0.37 + 0.11)
    loss = (out["pooler_output"] * cw(out["pooler_output"])).sum()
    loss = loss + 0.01 * (out["last_hidden_state"] * cw(out["last_hidden_state"])).sum()
    for i in tap_ids:
        h = out["hidden_states"][i]
        loss = loss + 0.01 * (h * cw(h)).sum()
    return loss


def _run_case(pkg, m, mode, hidden_state_ids=None):
    cfg = pkg.get_config(m["config"])
    model = _build(pkg, cfg, m["seed"], mode)
    x = pkg.weights.seeded_pixels(m["batch"], m["res_h"], m["res_w"], seed=m["seed"] + 1000).cuda()
    if hidden_state_ids is None:
        out = model(pixel_values=x, output_hidden_states=True, interpolate_pos_encoding=m["interp"])
        hs = dict(enumerate(out.hidden_states))
    else:
        out = model(pixel_values=x, hidden_state_ids=list(hidden_state_ids), interpolate_pos_encoding=m["interp"])
        hs = dict(zip(hidden_state_ids, out.hidden_states))
    loss = _probe_loss({"pooler_output": out.pooler_output, "last_hidden_state": out.last_hidden_state,
                        "hidden_states": hs}, m["taps"])
    loss.backward()
    tensors = {"pooler_output": out.pooler_output, "last_hidden_state": out.last_hidden_state}
    for i, h in hs.items():
        tensors[f"hidden_states.{i}"] = h
    named = dict(model.named_parameters())
    return tensors, named, loss.item()


def _check_against_fp16ac(rec, ac, tensors, named, label, bf16_bar=()):
    """2x rel-L2 / 3x max-err of HF under fp16 autocast; prefixes in `bf16_bar` only have to be within 2x / 3x of HF
    under BF16 autocast (see test_fp16_full_depth_so400m_384)."""
    ratios = {}
    items = dict(tensors)
    for k in rec:
        if k.startswith("grad.") and k.endswith(".shape"):
            name = k[len("grad."):-len(".shape")]
            items["grad." + name] = named[name].grad
    for prefix, t in items.items():
        if prefix + ".shape" not in rec or prefix.endswith("k_proj.bias"):
            continue   # k_proj.bias: exactly zero in real arithmetic, both sides are rounding noise
        mx, l2 = gu.err_stats(rec, prefix, t.detach().float().cpu())
        hf_l2, hf_mx = float(ac["fp16ac." + prefix + ".l2rel"]), float(ac["fp16ac." + prefix + ".maxerr"])
        ratios[prefix] = (l2 / (hf_l2 + 1e-12), mx / (hf_mx + 1e-12), l2, hf_l2)
    fails = []
    for prefix, (r_l2, r_mx, l2, hf_l2) in ratios.items():
        tag = "bf16ac." if prefix in bf16_bar else "fp16ac."
        bar_l2, bar_mx = float(ac[tag + prefix + ".l2rel"]), float(ac[tag + prefix + ".maxerr"])
        mx = r_mx * (float(ac["fp16ac." + prefix + ".maxerr"]) + 1e-12)
        if l2 > 2.0 * bar_l2 + 1e-5 or mx > 3.0 * bar_mx + 1e-6:
            fails.append(f"{prefix}: rel-L2 {l2:.3e} / max {mx:.3e} vs HF {tag[:4]} autocast {bar_l2:.3e} / {bar_mx:.3e}")
    assert not fails, f"{label}: " + "; ".join(fails)
    return ratios


@pytest.mark.parametrize("case", gu.CASES)
def test_fp16_error_within_2x_of_hf_fp16_autocast(case, pkg, hiplib):
    """|HIP_fp16 - fp32 golden| <= 2x (rel-L2) / 3x (max) |HF_fp16_autocast - fp32 golden| for pooled, last, every tap and
    every recorded gradient; and HIP-fp16's pooled / last errors <= 0.3x HIP-bf16's on the same inputs."""
    _check_fp16_case(case, pkg)


@pytest.mark.parametrize("case", gu.RECT_CASES)
def test_fp16_rectangular_error_within_2x_of_hf_fp16_autocast(case, pkg, hiplib):
    """The same yardstick and bars on rectangular images (rectangular position-table resize and its gradient)."""
    _check_fp16_case(case, pkg)


def _check_fp16_case(case, pkg):
    rec = gu.load(case)
    ac = dict(np.load(os.path.join(FP16_DIR, case + ".npz")))
    m = gu.meta(rec)
    tensors, named, _ = _run_case(pkg, m, "fp16")
    ratios = _check_against_fp16ac(rec, ac, tensors, named, case)
    tb, _, _ = _run_case(pkg, m, "bf16")
    vs_bf16 = {}
    for prefix in ("pooler_output", "last_hidden_state"):
        e16 = gu.err_stats(rec, prefix, tensors[prefix].detach().float().cpu())[1]
        eb = gu.err_stats(rec, prefix, tb[prefix].detach().float().cpu())[1]
        vs_bf16[prefix] = e16 / eb
        assert e16 <= 0.3 * eb, f"{prefix}: fp16 rel-L2 {e16:.3e} vs bf16 {eb:.3e}"
    acts = [v[0] for k, v in ratios.items() if not k.startswith("grad.")]
    grads = [v[0] for k, v in ratios.items() if k.startswith("grad.")]
    worst = max(ratios.items(), key=lambda kv: kv[1][0])
    print(f"[{case}] HIP-fp16 / HF-fp16-autocast rel-L2 ratio: activations max {max(acts):.2f}, gradients max "
          f"{max(grads):.2f} (worst {worst[0]}: {worst[1][2]:.2e} vs {worst[1][3]:.2e}); HIP fp16/bf16 error: pooled "
          f"{vs_bf16['pooler_output']:.3f}, last {vs_bf16['last_hidden_state']:.3f}")


def test_fp16_full_depth_so400m_384(pkg, hiplib):
    """All 27 blocks of so400m-patch14-384, B=1, forward and backward, against HF fp32 with the fp16-autocast bars."""
    rec = dict(np.load(os.path.join(FP16_DIR, "so400m27_384.npz")))
    m = gu.meta(rec)
    tensors, named, loss = _run_case(pkg, m, "fp16", hidden_state_ids=m["taps"])
    # q_proj gradient of block 13: dQ = dS.K with dS = P (dP - delta), delta = rowsum(dO o O) taken from the
    # fp16-ROUNDED attention output (the flash-attention identity; HF's eager backward takes sum(P o dP) instead).  Where
    # attention is near-uniform the true dS is tiny and that rounding (2^-11 of |dO||O|) dominates it; measured 1.3e-2
    # rel-L2 at block 13 against HF-fp16's 3.5e-3 (HF-bf16: 1.6e-2; block 26: 9.8e-3 vs 9.0e-3).  That one keeps the
    # bf16-autocast bar.
    deep_q = ("grad.encoder.layers.13.self_attn.q_proj.weight",)
    ratios = _check_against_fp16ac(rec, rec, tensors, named, "so400m27_384", bf16_bar=deep_q)
    pooled_abs = gu.err_stats(rec, "pooler_output", tensors["pooler_output"].detach().float().cpu())[0]
    print("[full depth fp16] pooled max|err| %.2e (HF fp16 autocast %.2e, bf16 autocast %.2e); HIP/HF rel-L2 | max "
          "ratios: " % (pooled_abs, float(rec["fp16ac.pooler_output.maxerr"]), float(rec["bf16ac.pooler_output.maxerr"]))
          + ", ".join(f"{k.replace('encoder.layers.', 'L')} {v[0]:.2f}|{v[1]:.2f} ({v[2]:.2e})" for k, v in ratios.items())
          + f"; loss {loss:.5f} vs {float(rec['loss']):.5f}")
    assert len(ratios) == 12


# ---------------------------------------------------------------------------------------------------------------------
# cifake-style training: fp16 autocast + GradScaler + FusedAdamW
# ---------------------------------------------------------------------------------------------------------------------
def _frozen(name, freeze_below):
    return freeze_below > 0 and (name.startswith("embeddings.") or
                                 any(name.startswith(f"encoder.layers.{i}.") for i in range(freeze_below)))


@pytest.mark.parametrize("freeze_below", [0, 1])
def test_fp16_autocast_gradscaler_training(pkg, oracle, hiplib, freeze_below):
    """create_model_and_transforms(compute_dtype="fp16") + a linear head, trained the way cifake_binary_classifier.py does
    (autocast fp16, scaler.scale(loss).backward(), unscale_, clip_grad_norm_, scaler.step, scaler.update), three steps
    against the fp32 CPU oracle with torch.optim.AdamW; then one step whose scaled gradients overflow fp16: the scaler
    finds the inf, skips the step (parameters and outputs bitwise unchanged) and lowers the scale."""
    cfg = pkg.get_config("hostile")
    seed, B = 11, 4
    lr, wd, clip = 2e-3, 0.05, 1.0
    torch.manual_seed(0)
    head0 = torch.nn.Linear(cfg.hidden_size, 1)
    x = pkg.weights.seeded_pixels(B, cfg.image_size, cfg.image_size, seed=5)
    y = torch.tensor([[0.0], [1.0], [1.0], [0.0]])

    # CPU reference: fp32 oracle encoder + fp32 head, torch AdamW, same clip
    sd0 = pkg.weights.seeded_state_dict(cfg, seed=seed)
    ref = {k: v.clone().requires_grad_(not _frozen(k, freeze_below)) for k, v in sd0.items()}
    rhead = torch.nn.Linear(cfg.hidden_size, 1)
    rhead.load_state_dict(head0.state_dict())
    rparams = [v for v in ref.values() if v.requires_grad] + list(rhead.parameters())
    ropt = torch.optim.AdamW(rparams, lr=lr, weight_decay=wd)
    ref_losses = []
    for _ in range(3):
        out = oracle.vision_forward(x, ref, cfg, False, False)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(rhead(out["pooler_output"]), y)
        ropt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(rparams, clip)
        ropt.step()
        ref_losses.append(loss.item())

    model, _, _ = pkg.create_model_and_transforms("hostile", device="cuda", compute_dtype="fp16", seed=seed)
    assert model.visual.compute_dtype == "fp16"
    for n, p in model.visual.named_parameters():
        p.requires_grad = not _frozen(n, freeze_below)
    head = torch.nn.Linear(cfg.hidden_size, 1).cuda()
    head.load_state_dict(head0.state_dict())
    params = [p for p in model.parameters() if p.requires_grad] + list(head.parameters())
    opt = pkg.FusedAdamW(params, lr=lr, weight_decay=wd).attach_encoder(model.visual)
    scaler = torch.amp.GradScaler("cuda")
    xd, yd = x.cuda(), y.cuda()

    def step(scaler):
        with torch.amp.autocast("cuda"):
            logits = head(model.encode_image(xd))
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.float(), yd)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(params, clip)
        scaler.step(opt)
        scaler.update()
        return loss.item()

    losses = [step(scaler) for _ in range(3)]
    rel = [abs(a - b) / abs(b) for a, b in zip(losses, ref_losses)]
    got = {k[len("vision_model."):]: v for k, v in model.visual.state_dict().items()}
    worst, who = 0.0, None
    for k, v in ref.items():
        if not v.requires_grad:
            assert torch.equal(got[k].cpu(), sd0[k]), k
            continue
        if k.endswith("k_proj.bias"):
            continue   # exactly-zero gradient in real arithmetic: Adam moves it by +-lr on noise (see test_train_loop_gpu)
        diff, moved = got[k].cpu() - v.detach(), v.detach() - sd0[k]
        if k == "head.attention.in_proj_bias":
            diff[cfg.hidden_size:2 * cfg.hidden_size] = 0
        r = diff.norm().item() / (moved.norm().item() + 1e-12)
        if r > worst:
            worst, who = r, k
    print(f"[fp16 GradScaler train freeze={freeze_below}] loss rel errs {[f'{e:.2e}' for e in rel]}, worst "
          f"moved-relative {worst:.3e} ({who}), scale {scaler.get_scale():.0f}")
    assert ref_losses[2] < ref_losses[0]
    # 2x the measured values (loss 7.1e-3 at step 3, where the loss itself is 1.3e-3; moved-relative 8.1e-2)
    assert max(rel) <= 1.5e-2, (losses, ref_losses)
    assert worst <= 0.17, (worst, who)

    # an overflowing step: scaled gradients far past fp16's range
    over = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    hbefore = {k: v.detach().clone() for k, v in head.state_dict().items()}
    with torch.no_grad():
        f0 = model.encode_image(xd).clone()
    step(over)
    # GradScaler.update() halves the scale exactly when unscale_ found an inf / NaN
    assert over.get_scale() == 2.0 ** 39, "the scaler must find the overflow and back off"
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed in a skipped step"
    for k, v in head.state_dict().items():
        assert torch.equal(v, hbefore[k]), k
    with torch.no_grad():
        f1 = model.encode_image(xd)
    assert torch.equal(f0, f1), "forward after the skipped step differs"


# ---------------------------------------------------------------------------------------------------------------------
# surfaces
# ---------------------------------------------------------------------------------------------------------------------
def test_fp16_patch_operand_matches_pixels(pkg, hiplib):
    cfg = pkg.get_config("so400m-1layer")
    model, _, _ = pkg.create_model_and_transforms("so400m-1layer", device="cuda", compute_dtype="fp16", seed=3)
    torch.manual_seed(3)
    img = torch.rand(2, 3, cfg.image_size, cfg.image_size, device="cuda")
    ops = pkg.preprocess.to_patch_operand(img, cfg, compute_dtype="fp16")
    assert ops.data.dtype == torch.float16
    with torch.no_grad():
        a = model.encode_image(patches=ops)
        b = model.encode_image((img - 0.5) / 0.5)
    bitwise = torch.equal(a, b)
    print(f"[fp16 patches vs pixels] bitwise {bitwise}, max|diff| {(a - b).abs().max().item():.2e}")
    assert relerr(a, b) < 2e-3
    bad = pkg.preprocess.to_patch_operand(img, cfg, compute_dtype="bf16")
    with pytest.raises(Exception):
        model.encode_image(patches=bad)


def test_fp16_backward_is_bitwise_reproducible(pkg, hiplib):
    cfg = pkg.get_config("so400m-1layer")
    model = _build(pkg, cfg, 9, "fp16")
    x = pkg.weights.seeded_pixels(2, 384, 384, seed=10).cuda()
    grads = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        out = model(pixel_values=x)
        (out.pooler_output.square().sum() + out.last_hidden_state.mean()).backward()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    for n in grads[0]:
        assert torch.isfinite(grads[0][n]).all(), n
        assert torch.equal(grads[0][n], grads[1][n]), n
