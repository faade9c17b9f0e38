"""GPU tests of the MX-fp8 inference mode (compute_dtype="mxfp8", SGL_DTYPE_MXFP8).

The four projection GEMMs of every block read MX-fp8 operands (e4m3fn, one E8M0 scale per 32 K-elements) on
v_mfma_scale_f32_16x16x128_f8f6f4; everything else is the bf16 mode.  Bars:

  * quantize (standalone and LayerNorm -> MX): bit-exact against tests/mx_ref.py, or, where the kernel quantizes its own
    fp32 result (LN, the fc1 GELU epilogue), >= 99.9 % of the bytes equal to the reference quantizer applied to the fp64
    result and the rest within one e4m3 step;
  * MX GEMM: against an fp64 product of the DEQUANTIZED operands, so only the accumulation remains;
  * encoder: against (i) a float64 emulation of the mode (reference quantizer on both operands of the four block GEMMs,
    the bf16 stages rounded, everything else exact) and (ii) the exact forward; (i) must stay below (ii): the error is the
    format's, not the kernels'.
"""
import copy
import math

import pytest
import torch

import golden_util as gu
import mx_ref

pytestmark = pytest.mark.gpu

BF16 = 1
EPI_BIAS_GELU, EPI_RES_F32, EPI_QKV = 1, 2, 3


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


def kpad(K):
    return (K + 127) // 128 * 128


def quantize_gpu(lib, x, Kp=None):
    M, K = x.shape
    Kp = Kp or kpad(K)
    q = torch.full((M, Kp), 0xAB, dtype=torch.uint8, device="cuda")
    s = torch.full((M, Kp // 32), 0xAB, dtype=torch.uint8, device="cuda")
    code = {torch.float32: 0, torch.bfloat16: BF16}[x.dtype]
    ok(lib.sgl_op_quantize_mxfp8(P(x), code, x.stride(0), M, K, Kp, P(q), P(s), stream()))
    torch.cuda.synchronize()
    return q, s


def gelu_tanh(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


def byte_agreement(q, s, q_ref, s_ref, abs_floor=0.0):
    """(fraction of equal element bytes, max distance of the differing ones in e4m3 steps, or in units of abs_floor where
    that is larger)."""
    same = (q == q_ref).double().mean().item()
    v, vr = mx_ref.dequantize(q, s), mx_ref.dequantize(q_ref, s_ref)
    # one step at a value's binade: 2^(floor(log2 |v|) - 3), at least the subnormal step 2^-9, in the block's scale
    sc = torch.maximum(s, s_ref).to(torch.float64).repeat_interleave(32, dim=1) - 127.0
    mag = torch.maximum(v.abs(), vr.abs()) * torch.pow(2.0, -sc)
    step = torch.pow(2.0, torch.floor(torch.log2(torch.clamp(mag, min=2.0 ** -6))) - 3.0) * torch.pow(2.0, sc)
    d = ((v - vr).abs() / torch.clamp(step, min=abs_floor))
    return same, d.max().item()


# ---------------------------------------------------------------------------------------------------------------------
# quantizer
# ---------------------------------------------------------------------------------------------------------------------
def _hostile_rows(K, gen):
    rows = [torch.randn(K, generator=gen), torch.zeros(K), torch.randn(K, generator=gen) * 1e30,
            torch.randn(K, generator=gen) * 1e-30, torch.randn(K, generator=gen) * 1e-42]
    r = torch.randn(K, generator=gen) * 0.1
    r[::32] = 448.0                                   # amax exactly on a 448 * 2^e boundary
    rows.append(r)
    r = torch.randn(K, generator=gen) * 0.1
    r[::32] = float(torch.nextafter(torch.tensor(448.0 * 4), torch.tensor(1e9)))   # just past one
    rows.append(r)
    r = torch.randn(K, generator=gen)
    r[1::7] = 0.0
    r[::5] *= 1e-6                                    # subnormal e4m3 elements within a block
    rows.append(r)
    r = torch.randn(K, generator=gen) * torch.logspace(-20, 20, K)
    rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("K", [32, 64, 100, 144, 538, 1152, 4304])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_bit_exact(lib, K, dtype):
    gen = torch.Generator().manual_seed(K)
    x = torch.cat([_hostile_rows(K, gen), torch.randn(300, K, generator=gen) * 3]).to(dtype)
    q, s = quantize_gpu(lib, x.cuda())
    q_ref, s_ref = mx_ref.quantize(x)
    assert torch.equal(s.cpu(), s_ref), (s.cpu() != s_ref).nonzero()[:5]
    assert torch.equal(q.cpu(), q_ref), (q.cpu() != q_ref).nonzero()[:5]


def test_quantize_strided_input(lib):
    x = torch.randn(37, 300, device="cuda")
    q, s = quantize_gpu(lib, x[:, :200])
    q_ref, s_ref = mx_ref.quantize(x[:, :200].cpu())
    assert torch.equal(q.cpu(), q_ref) and torch.equal(s.cpu(), s_ref)


def test_quantize_non_finite_block(lib):
    x = torch.randn(4, 256, device="cuda")
    x[1, 40] = float("inf")
    x[2, 200] = float("nan")
    q, s = quantize_gpu(lib, x)
    q_ref, s_ref = mx_ref.quantize(x.cpu())
    assert torch.equal(q.cpu(), q_ref) and torch.equal(s.cpu(), s_ref)
    assert s[1, 1].item() == 0xFF and s[2, 6].item() == 0xFF and (q[1, 32:64] == 0x7F).all()


# ---------------------------------------------------------------------------------------------------------------------
# MX GEMM
# ---------------------------------------------------------------------------------------------------------------------
NT_SHAPES = [(93312, 1152, 1152), (2916, 3456, 1152), (2916, 4352, 1152), (2916, 1152, 4352), (2300, 4352, 1152),
             (2051, 1160, 200), (729, 1152, 1152), (300, 1152, 4352), (64, 4352, 1152), (200, 136, 72), (1, 8, 8),
             (1, 1152, 1152), (729, 4352, 1152), (333, 432, 144), (333, 144, 538)]
# fp32 output: the accumulation alone (the MFMA's product sums against fp64);  bf16 output: plus bf16 rounding.
# v_mfma_scale_f32_16x16x128_f8f6f4 does not sum its 128 products as an fp32 chain (on exact integer-valued data with
# per-lane scales its error is ~1e-4 of sum|a.b|, thousands of fp32 ulps): measured max err / max|ref| 1.0e-5 .. 3.1e-5
# over NT_SHAPES (the largest at K = 200 and M = 1), so the bar is 2x the largest; bf16 outputs measured <= 2.9e-3.
TOL_F32_OUT, TOL_BF16_OUT = 6.2e-5, 6e-3
# MX outputs quantized in a kernel (fc1 GELU epilogue, LayerNorm): measured 0.0757-0.0924 % of the bytes differ from the
# reference quantizer applied to the fp64 result (the accumulation error above moves values across rounding midpoints and
# 448 * 2^e boundaries), so at most 0.2 % may differ (2x); a differing byte's value is within one e4m3 step, or within 2x
# the accumulation bar of max|x| (near zero the e4m3 subnormal step of a block, 2^(e-9), is finer than that error)
MAX_DIFF_BYTES = 0.002


def _operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, K, device="cuda", generator=g)
    B = torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)
    return A, B


def _gemm(lib, Aq, As, Bq, Bs, M, N, Kp, epi, out, ldo, out_sc=None, bias=None, res=None, ldr=0, tokens=1, heads=1,
          hd=8, hdp=8, batch=1):
    return lib.sgl_op_gemm_nt_mx(P(Aq), P(As), P(Bq), P(Bs), M, N, Kp, epi, P(out), ldo, P(out_sc), P(bias), P(res), ldr,
                                 tokens, heads, hd, hdp, batch, stream())


def _relerr(got, ref):
    return ((got.double() - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_mx_res_f32(lib, M, N, K):
    A, B = _operands(M, N, K, M + N + K)
    Aq, As = quantize_gpu(lib, A)
    Bq, Bs = quantize_gpu(lib, B)
    Kp = Aq.shape[1]
    bias = torch.randn(N, device="cuda")
    res = torch.randn(M, N, device="cuda")
    out = torch.full((M, N), float("nan"), device="cuda")
    ok(_gemm(lib, Aq, As, Bq, Bs, M, N, Kp, EPI_RES_F32, out, N, bias=bias, res=res, ldr=N))
    acc = mx_ref.dequantize(Aq, As) @ mx_ref.dequantize(Bq, Bs).t()
    err = _relerr(out - res, acc + bias.double())
    print(f"[mx gemm {M}x{N}x{K}] RES_F32 max err / max|ref| {err:.2e}")
    assert err <= TOL_F32_OUT


@pytest.mark.parametrize("batch,tokens,heads,hd", [(2, 9, 2, 72), (3, 729, 16, 72), (11, 196, 12, 64), (2, 9, 2, 8)])
def test_gemm_nt_mx_qkv_scatter(lib, batch, tokens, heads, hd):
    M, D = batch * tokens, heads * hd
    N = 3 * D
    hdp = (hd + 15) // 16 * 16
    A, B = _operands(M, N, D, M + D)
    Aq, As = quantize_gpu(lib, A)
    Bq, Bs = quantize_gpu(lib, B)
    bias = torch.randn(N, device="cuda")
    out = torch.full((3, batch, heads, tokens, hdp), float("nan"), device="cuda", dtype=torch.bfloat16)
    ok(_gemm(lib, Aq, As, Bq, Bs, M, N, Aq.shape[1], EPI_QKV, out, 0, bias=bias, tokens=tokens, heads=heads, hd=hd,
             hdp=hdp, batch=batch))
    ref = mx_ref.dequantize(Aq, As) @ mx_ref.dequantize(Bq, Bs).t() + bias.double()
    ref = ref.view(batch, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4)
    err = _relerr(out[..., :hd], ref)
    print(f"[mx qkv {batch}x{tokens}x{heads}x{hd}] max err / max|ref| {err:.2e}")
    assert err <= TOL_BF16_OUT
    assert (out[..., hd:] == 0).all()


@pytest.mark.parametrize("M,N,K", [(2916, 4352, 1152), (729, 4352, 1152), (1, 4352, 1152), (333, 640, 144),
                                   (2051, 128, 200)])
def test_gemm_nt_mx_gelu_to_mx(lib, M, N, K):
    A, B = _operands(M, N, K, 7 * M + N)
    Aq, As = quantize_gpu(lib, A)
    Bq, Bs = quantize_gpu(lib, B)
    bias = torch.randn(N, device="cuda") * 0.5
    ldo = kpad(N)
    out = torch.full((M, ldo), 0xAB, dtype=torch.uint8, device="cuda")
    osc = torch.full((M, ldo // 32), 0xAB, dtype=torch.uint8, device="cuda")
    ok(_gemm(lib, Aq, As, Bq, Bs, M, N, Aq.shape[1], EPI_BIAS_GELU, out, ldo, out_sc=osc, bias=bias))
    u = mx_ref.dequantize(Aq, As) @ mx_ref.dequantize(Bq, Bs).t() + bias.double()
    q_ref, s_ref = mx_ref.quantize(gelu_tanh(u), Kp=ldo)
    a = gelu_tanh(u)
    same, steps = byte_agreement(out[:, :N], osc[:, :N // 32], q_ref[:, :N].cuda(), s_ref[:, :N // 32].cuda(),
                                 abs_floor=2 * TOL_F32_OUT * a.abs().max().item())
    print(f"[mx gelu {M}x{N}x{K}] equal bytes {same:.5f}, max distance {steps:.2f} steps")
    assert same >= 1 - MAX_DIFF_BYTES and steps <= 1.0 + 1e-9


def test_gemm_nt_mx_non_finite_propagates(lib):
    M, N, K = 200, 256, 384
    A, B = _operands(M, N, K, 3)
    A[17, 70] = float("inf")           # block 2 of row 17
    B[5, 300] = float("nan")           # block 9 of column 5
    Aq, As = quantize_gpu(lib, A)
    Bq, Bs = quantize_gpu(lib, B)
    bias = torch.zeros(N, device="cuda")
    res = torch.zeros(M, N, device="cuda")
    out = torch.zeros(M, N, device="cuda")
    ok(_gemm(lib, Aq, As, Bq, Bs, M, N, Aq.shape[1], EPI_RES_F32, out, N, bias=bias, res=res, ldr=N))
    nan = torch.isnan(out)
    assert nan[17].all() and nan[:, 5].all()
    nan[17] = False
    nan[:, 5] = False
    assert not nan.any() and torch.isfinite(out[~torch.isnan(out)]).all()


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm -> MX
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", [(5832, 1152), (729, 1152), (1, 1152), (333, 144), (100, 64), (50, 768), (20, 2048)])
def test_layernorm_fwd_mx(lib, M, D):
    torch.manual_seed(M + D)
    x = torch.randn(M, D, device="cuda") * 3 + torch.randn(D, device="cuda")
    x[:, 7] *= 40.0                                        # one outlier channel
    g = torch.randn(D, device="cuda")
    b = torch.randn(D, device="cuda") * 0.1
    Kp = kpad(D)
    q = torch.full((M, Kp), 0xAB, dtype=torch.uint8, device="cuda")
    s = torch.full((M, Kp // 32), 0xAB, dtype=torch.uint8, device="cuda")
    ok(lib.sgl_op_layernorm_fwd_mx(P(x), P(g), P(b), P(q), P(s), M, D, Kp, 1e-6, stream()))
    xd = x.double()
    y = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-6) * g.double() \
        + b.double()
    q_ref, s_ref = mx_ref.quantize(y.cpu(), Kp=Kp)
    same, steps = byte_agreement(q, s, q_ref.cuda(), s_ref.cuda())
    print(f"[ln mx {M}x{D}] equal bytes {same:.5f}, max distance {steps:.2f} steps")
    assert same >= 1 - MAX_DIFF_BYTES and steps <= 1.0 + 1e-9
    assert (q[:, D:] == 0).all() and (s[:, (D + 31) // 32:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _emulated_forward(oracle, pixels, sd, cfg, interp, mx=True):
    """float64 forward: the oracle's ops, with (mx=True) the mode's arithmetic: the reference quantizer on both operands of
    the four block GEMMs, and the bf16 roundings of the stages the mode keeps in bf16 (patch-GEMM operands, the QKV
    projection's output, the attention output).  Those roundings (2^-9) matter: re-quantization turns a perturbation d of
    an operand into byte flips of one e4m3 step (2^-4) on a fraction ~d / 2^-4 of its elements, i.e. an rms error of
    order sqrt(d * 2^-4) ~ 1 %, so an emulation without them differs from the kernels by nearly the format's own error."""
    cd = cfg.to_dict() if not isinstance(cfg, dict) else cfg
    fq = mx_ref.fake_quant if mx else (lambda t: t)
    rb = _bf16 if mx else (lambda t: t)
    if mx:
        sd = dict(sd)
        sd["embeddings.patch_embedding.weight"] = _bf16(sd["embeddings.patch_embedding.weight"])
    x = oracle.patch_embed(rb(pixels), sd, cd, interp)
    eps, nh = cd["layer_norm_eps"], cd["num_attention_heads"]

    def lin(h, w, b):
        return fq(h) @ fq(w).t() + b

    for l in range(cd["num_hidden_layers"]):
        pre = f"encoder.layers.{l}."
        bsz, n, d = x.shape
        dh = d // nh
        h = oracle.layer_norm(x, sd[pre + "layer_norm1.weight"], sd[pre + "layer_norm1.bias"], eps)
        a = pre + "self_attn."
        q, k, v = (rb(lin(h, sd[a + f"{t}_proj.weight"], sd[a + f"{t}_proj.bias"])).view(bsz, n, nh, dh).transpose(1, 2)
                   for t in "qkv")
        pr = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, dim=-1)
        o = rb((pr @ v).transpose(1, 2).reshape(bsz, n, d))
        x = x + lin(o, sd[a + "out_proj.weight"], sd[a + "out_proj.bias"])
        h = oracle.layer_norm(x, sd[pre + "layer_norm2.weight"], sd[pre + "layer_norm2.bias"], eps)
        u = oracle.gelu_tanh(lin(h, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"]))
        x = x + lin(u, sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"])
    last = oracle.layer_norm(x, sd["post_layernorm.weight"], sd["post_layernorm.bias"], eps)
    pooled = oracle.pooling_head(last, sd, cd) if cd.get("vision_use_head", True) else None
    return pooled, last


def _rel_l2(got, ref):
    got, ref = got.detach().double().reshape(-1), ref.detach().double().to(got.device).reshape(-1)
    return ((got - ref).norm() / ref.norm()).item()


def _encoder_errors(pkg, oracle, cfg, seed, B, res, interp):
    sd = pkg.weights.seeded_state_dict(cfg, seed=seed)
    x = pkg.weights.seeded_pixels(B, res, res, seed=seed + 1000)
    dev = "cpu" if interp else "cuda"     # the oracle's position-table resize builds its tables on the CPU
    sd64 = {k: v.double().to(dev) for k, v in sd.items()}
    x64 = x.double().to(dev)
    with torch.no_grad():
        e_pool, e_last = _emulated_forward(oracle, x64, sd64, cfg, interp, mx=True)
        r_pool, r_last = _emulated_forward(oracle, x64, sd64, cfg, interp, mx=False)
        errs = {}
        for mode in ("mxfp8", "bf16"):
            m = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode)
            m.load_state_dict(sd)
            m = m.cuda()
            out = m(pixel_values=x.cuda(), interpolate_pos_encoding=interp)
            errs[mode] = {"emul_pool": _rel_l2(out.pooler_output, e_pool), "emul_last": _rel_l2(out.last_hidden_state, e_last),
                          "ref_pool": _rel_l2(out.pooler_output, r_pool), "ref_last": _rel_l2(out.last_hidden_state, r_last)}
    errs["format"] = {"pool": _rel_l2(e_pool, r_pool), "last": _rel_l2(e_last, r_last)}
    return errs


# Bars, relative to the format's own error ('format': the float64 emulation of the mode against the exact forward, same
# inputs, rel-L2 of pooled and last_hidden_state):
#   (i)  HIP mxfp8 vs the emulation <= 0.75x the format's error: the kernels follow the format's rounding, they do not add an
#        error of their own.  Measured 0.15-0.21x (pooled) and 0.40-0.56x (last) on the golden cases, 0.20x / 0.49x at full
#        depth.  It does not go to zero because re-quantization turns every perturbation the emulation does not reproduce
#        bit for bit (the bf16 attention kernel's own roundings, fp32 LayerNorm statistics, the MFMA's accumulation) into
#        one-step byte flips (see _emulated_forward); an independent draw of the format's noise would sit near 1.4x.
#   (ii) HIP mxfp8 vs the exact forward <= 2x the format's error (measured 0.99-1.04x).
# The bf16 mode's error on the same inputs is printed next to it (mxfp8 is 8-16x the bf16 error on seeded weights).
def _check_encoder(errs, label):
    print(f"[mxfp8 {label}] " + str({k: {kk: f"{vv:.2e}" for kk, vv in v.items()} for k, v in errs.items()}))
    mx, fmt = errs["mxfp8"], errs["format"]
    for t in ("pool", "last"):
        assert math.isfinite(mx[f"ref_{t}"])
        assert mx[f"emul_{t}"] <= 0.75 * fmt[t], (label, t)
        assert mx[f"ref_{t}"] <= 2.0 * fmt[t], (label, t)


@pytest.mark.parametrize("case", gu.CASES)
def test_mxfp8_encoder_golden_cases(case, pkg, oracle, hiplib):
    m = gu.meta(gu.load(case))
    cfg = pkg.get_config(m["config"])
    _check_encoder(_encoder_errors(pkg, oracle, cfg, m["seed"], m["batch"], m["res"], m["interp"]), case)


def test_mxfp8_encoder_full_depth_so400m_384(pkg, oracle, hiplib):
    cfg = pkg.get_config("so400m-patch14-384")
    _check_encoder(_encoder_errors(pkg, oracle, cfg, 0, 2, 384, False), "full depth so400m@384 B=2")


# ---------------------------------------------------------------------------------------------------------------------
# frozen-backbone training, refusal, reproducibility
# ---------------------------------------------------------------------------------------------------------------------
def _model(pkg, name="hostile", seed=7):
    cfg = pkg.get_config(name)
    m = pkg.SiglipVisionModelHIP(cfg, compute_dtype="mxfp8")
    m.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=seed))
    return m.cuda(), cfg


def test_frozen_backbone_head_training(pkg, hiplib):
    enc, cfg = _model(pkg)
    x = pkg.weights.seeded_pixels(3, 42, 42, seed=5).cuda()
    torch.manual_seed(0)
    head = torch.nn.Linear(cfg.hidden_size, 2).cuda()
    head2 = copy.deepcopy(head)
    y = torch.tensor([0, 1, 1], device="cuda")
    # trainable encoder: refused
    with pytest.raises(RuntimeError, match="bf16"):
        enc(pixel_values=x, interpolate_pos_encoding=True)
    enc.requires_grad_(False)
    # grad-enabled forward, frozen encoder, trainable head
    opt = torch.optim.SGD(head.parameters(), lr=0.1)
    feats = enc(pixel_values=x, interpolate_pos_encoding=True).pooler_output
    loss = torch.nn.functional.cross_entropy(head(feats), y)
    loss.backward()
    opt.step()
    # the same step driven by the mode's own detached features
    with torch.no_grad():
        f2 = enc(pixel_values=x, interpolate_pos_encoding=True).pooler_output
    opt2 = torch.optim.SGD(head2.parameters(), lr=0.1)
    torch.nn.functional.cross_entropy(head2(f2.detach()), y).backward()
    opt2.step()
    assert torch.equal(head.weight, head2.weight) and torch.equal(head.bias, head2.bias)
    # one trainable encoder parameter is enough to refuse
    enc.encoder.layers[1].mlp.fc1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="freeze"):
        enc(pixel_values=x, interpolate_pos_encoding=True)


def test_mxfp8_reproducible_and_requantizes_on_load(pkg, hiplib):
    enc, cfg = _model(pkg, "so400m-patch14-384", seed=0)
    cfg_small = pkg.get_config("hostile")
    x = pkg.weights.seeded_pixels(2, 384, 384, seed=3).cuda()
    with torch.no_grad():
        a = enc(pixel_values=x, output_hidden_states=True)
        b = enc(pixel_values=x, output_hidden_states=True)
        assert torch.equal(a.pooler_output, b.pooler_output) and torch.equal(a.last_hidden_state, b.last_hidden_state)
        assert all(torch.equal(h1, h2) for h1, h2 in zip(a.hidden_states, b.hidden_states))
        sd2 = pkg.weights.seeded_state_dict(cfg, seed=1)
        enc.load_state_dict(sd2)
        c = enc(pixel_values=x)
        assert not torch.equal(c.pooler_output, a.pooler_output)
        fresh = pkg.SiglipVisionModelHIP(cfg, compute_dtype="mxfp8")
        fresh.load_state_dict(sd2)
        d = fresh.cuda()(pixel_values=x)
        assert torch.equal(c.pooler_output, d.pooler_output) and torch.equal(c.last_hidden_state, d.last_hidden_state)
    assert cfg_small.hidden_size == 144


def test_mxfp8_patch_operand_matches_pixels(pkg, hiplib):
    """preprocess.to_patch_operand(compute_dtype="mxfp8") gives the bf16 patch operand the mode's patch GEMM reads."""
    cfg = pkg.get_config("so400m-1layer")
    model, _, _ = pkg.create_model_and_transforms("so400m-1layer", device="cuda", compute_dtype="mxfp8", seed=3)
    model.requires_grad_(False)
    torch.manual_seed(3)
    img = torch.rand(2, 3, cfg.image_size, cfg.image_size, device="cuda")
    ops = pkg.preprocess.to_patch_operand(img, cfg, compute_dtype="mxfp8")
    assert ops.data.dtype == torch.bfloat16
    with torch.no_grad():
        a = model.encode_image(patches=ops)
        b = model.encode_image((img - 0.5) / 0.5)
    print(f"[mxfp8 patches vs pixels] bitwise {torch.equal(a, b)}, max|diff| {(a - b).abs().max().item():.2e}")
    assert ((a - b).abs().max() / b.abs().max()).item() < 2e-2
