"""GPU: whole-model runs with token counts whose buffers cross 2^31 bytes, 2^32 bytes or 2^31 elements, every image checked.

Config so400m-1layer at 384 px (729 tokens per image), seeded weights and pixels.  The reference for image i is the same
library run on a chunk of 8 images that contains i: 8 x 729 = 5832 tokens >= 2048, so a chunk takes the same GEMM tile
dispatch as the big run, and small batches are held to the oracle elsewhere (tests/test_abi_contract_gpu.py,
tests/test_full_depth_configs_gpu.py).  Every forward kernel's per-row arithmetic is independent of the number of rows
(GEMM: K order per output row; LayerNorm: per row; attention: per (image, head); MX blocks: per row), and so is the
backward's dX chain, so the expected relation is BITWISE equality of last_hidden_state, pooler_output and the pixel gradient
for every image: test_batch_invariance_is_bitwise establishes it between 8 and 16 images, the large runs assert it chunk by
chunk on the device.  Parameter gradients are sums over all tokens in an order that depends on M: they are held to the 1e-4
relative norm of tests/test_recompute_gpu.py::test_recompute_large_token_count against the fp32 sum of the chunk runs.

A test skips only when torch.cuda.mem_get_info() shows less free memory than it computes it needs (sgl_query_sizes plus its
own tensors); on an idle MI355X none does.  Each prints its peak allocation and wall time."""
import time

import pytest
import torch

import attn_probs_ref as apr

pytestmark = pytest.mark.gpu

CFG, RES, N, D = "so400m-1layer", 384, 729, 1152
CHUNK = 8
# mode -> the smallest batch that crosses the extent the case is there for
INFER = {"bf16": 676,     # a [M][4352] bf16 4.29e9 B (0.1 % under the GEMM guard); V base above 2^31 B
         "fp16": 676,     # the same instantiations in fp16
         "fp32": 338,     # a fp32 4.29e9 B; gemm_f32 long indexing
         "bf16x3": 225,   # split operand [M][3 * 4352] bf16, 4.28e9 B
         "mxfp8": 1360}   # fp32 hidden slot 4.57e9 B and fp8 a 4.31e9 B above 2^32; K base above 2^31 B, V above 2^32 B
TRAIN = {"bf16": 676, "fp16": 676, "fp32": 338}


def _model(pkg, mode, recompute=False):
    cfg = pkg.get_config(CFG)
    m = pkg.SiglipVisionModelHIP(cfg, compute_dtype=mode, recompute=recompute)
    m.load_state_dict(pkg.weights.seeded_state_dict(cfg, seed=3))
    return m.cuda()


def _pixels(B, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(B, 3, RES, RES, device="cuda", generator=g) * 2 - 1


def _need_or_skip(m, B, train, recompute, extra):
    """Bytes the test is about to allocate: the library's arenas (sgl_query_sizes), the hidden states the package keeps,
    the same for one chunk, and the test's own tensors (`extra`)."""
    _, saved, ws = m._contexts.sizes(B, RES, RES, train, recompute)
    _, saved8, ws8 = m._contexts.sizes(CHUNK, RES, RES, train, recompute)
    hidden = 2 * B * N * D * 4
    need = saved + ws + saved8 + ws8 + hidden + extra
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB free")
    return need


def _chunks(B):
    """8-image chunks that cover [0, B); the last one is moved back so that it is 8 images too.  `new` is the first image
    of the chunk that no earlier chunk held."""
    out = []
    for lo in range(0, B, CHUNK):
        hi = min(B, lo + CHUNK)
        out.append((max(0, hi - CHUNK), hi, lo))
    return out


class _Report:
    def __init__(self, what):
        self.what = what
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()

    def done(self, note=""):
        torch.cuda.synchronize()
        print(f"\n[large-tokens] {self.what}: peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB, "
              f"{time.perf_counter() - self.t0:.2f} s {note}")


@pytest.mark.parametrize("mode", list(INFER))
def test_batch_invariance_is_bitwise(pkg, hiplib, mode):
    """8 against 16 images (both at or above 2048 tokens): outputs of the first 8 are bitwise those of the 8-image run, in
    inference for every mode and, where the mode trains, for the pixel gradient too."""
    m = _model(pkg, mode).eval()
    x = _pixels(16, seed=1)
    with torch.no_grad():
        big = m(pixel_values=x)
        small = m(pixel_values=x[:8])
    assert torch.equal(big.last_hidden_state[:8], small.last_hidden_state), f"{mode}: last_hidden_state depends on B"
    assert torch.equal(big.pooler_output[:8], small.pooler_output), f"{mode}: pooler_output depends on B"
    if mode in TRAIN:
        g = torch.Generator(device="cuda").manual_seed(2)
        wl = torch.randn(16, N, D, device="cuda", generator=g)
        wp = torch.randn(16, D, device="cuda", generator=g)
        grads = []
        for lo, hi in ((0, 16), (0, 8)):
            xi = x[lo:hi].clone().requires_grad_()
            o = m.train()(pixel_values=xi)
            ((o.last_hidden_state * wl[lo:hi]).sum() + (o.pooler_output * wp[lo:hi]).sum()).backward()
            grads.append(xi.grad)
        assert torch.equal(grads[0][:8], grads[1]), f"{mode}: pixel gradient depends on B"
    del big, small, x, m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", list(INFER))
def test_inference_every_image(pkg, hiplib, mode):
    """Inference through the workspace layout with two ping-pong hidden-state slots, at the batch of INFER: every image's
    last_hidden_state and pooler_output equal, bit for bit, those of an 8-image call on a chunk that contains it."""
    B = INFER[mode]
    m = _model(pkg, mode).eval()
    need = _need_or_skip(m, B, False, False, B * 3 * RES * RES * 4 + (B + CHUNK) * (N + 1) * D * 4)
    rep = _Report(f"inference {mode} B={B} ({B * N} tokens)")
    x = _pixels(B)
    with torch.no_grad():
        big = m(pixel_values=x)
        last, pooled = big.last_hidden_state, big.pooler_output
        del big
        assert bool(torch.isfinite(pooled).all())
        for lo, hi, _ in _chunks(B):
            ref = m(pixel_values=x[lo:hi])
            assert torch.equal(last[lo:hi], ref.last_hidden_state), f"{mode}: last_hidden_state of images {lo}..{hi - 1}"
            assert torch.equal(pooled[lo:hi], ref.pooler_output), f"{mode}: pooler_output of images {lo}..{hi - 1}"
            del ref
    rep.done(f"(computed need {need / 2**30:.1f} GiB)")
    del last, pooled, x, m
    torch.cuda.empty_cache()


def _train_every_image(pkg, mode, B, recompute):
    m = _model(pkg, mode, recompute=recompute).train()
    nparam = sum(p.numel() for p in m.parameters())
    # pixels and their gradient; upstream weights; the loss's products and their gradients; four sets of parameter gradients
    extra = 2 * B * 3 * RES * RES * 4 + 2 * B * (N + 1) * D * 4 + 2 * B * (N + 1) * D * 4 + 4 * nparam * 4
    need = _need_or_skip(m, B, True, recompute, extra)
    rep = _Report(f"training {mode}{' recompute' if recompute else ''} B={B} ({B * N} tokens)")
    g = torch.Generator(device="cuda").manual_seed(0)
    x = _pixels(B).requires_grad_()
    wl = torch.randn(B, N, D, device="cuda", generator=g)
    wp = torch.randn(B, D, device="cuda", generator=g)

    def run(px, lo, hi, new):
        for p in m.parameters():
            p.grad = None
        out = m(pixel_values=px)
        w_l, w_p = wl[lo:hi], wp[lo:hi]
        if new > lo:      # images an earlier chunk already counted: zero upstream gradient, so they add nothing
            w_l, w_p = w_l.clone(), w_p.clone()
            w_l[:new - lo] = 0
            w_p[:new - lo] = 0
        ((out.last_hidden_state * w_l).sum() + (out.pooler_output * w_p).sum()).backward()
        return out.last_hidden_state.detach(), out.pooler_output.detach()

    last, pooled = run(x, 0, B, 0)
    dx = x.grad
    full = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert bool(torch.isfinite(dx).all())
    acc = {n: torch.zeros_like(v) for n, v in full.items()}
    for lo, hi, new in _chunks(B):
        xi = x.detach()[lo:hi].clone().requires_grad_()
        l8, p8 = run(xi, lo, hi, new)
        assert torch.equal(last[lo:hi], l8), f"{mode}: last_hidden_state of images {lo}..{hi - 1}"
        assert torch.equal(pooled[lo:hi], p8), f"{mode}: pooler_output of images {lo}..{hi - 1}"
        assert torch.equal(dx[new:hi], xi.grad[new - lo:]), f"{mode}: pixel gradient of images {new}..{hi - 1}"
        for n, p in m.named_parameters():
            acc[n] += p.grad
        del xi, l8, p8
    worst_rel, worst_abs = 0.0, 0.0
    for n in full:
        rel = ((acc[n] - full[n]).norm() / full[n].norm().clamp_min(1e-30)).item()
        dev = ((acc[n] - full[n]).abs().max() / full[n].abs().max().clamp_min(1e-30)).item()
        worst_rel, worst_abs = max(worst_rel, rel), max(worst_abs, dev)
        assert rel <= 1e-4, (n, rel)
    rep.done(f"(computed need {need / 2**30:.1f} GiB; parameter gradients vs {len(_chunks(B))} accumulated chunks: worst "
             f"relative norm {worst_rel:.2e}, worst element deviation / max |grad| {worst_abs:.2e})")
    for p in m.parameters():
        p.grad = None
    del last, pooled, dx, full, acc, x, wl, wp, m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", list(TRAIN))
def test_plain_training_every_image(pkg, hiplib, mode):
    """Plain context (the only path that writes the GELU pre-activation u for every block into `saved`): outputs and the
    pixel gradient of every image bitwise equal to its 8-image chunk run, parameter gradients within 1e-4 (relative norm)
    of the fp32 sum of the chunk runs' gradients."""
    _train_every_image(pkg, mode, TRAIN[mode], False)


def test_recompute_training_every_image(pkg, hiplib):
    """The recompute context at B = 676: the same every-image check."""
    _train_every_image(pkg, "bf16", 676, True)


def test_output_attentions_bench_batch(pkg, hiplib):
    """output_attentions=True at the benchmark's batch (B = 128, bf16): 128 * 16 * 729 * 729 fp32 = 4.35e9 bytes for the
    layer, past 2^32.  Every (image, head) slab equals the slab from an 8-image call, and four slabs are within the
    float64 bound of tests/attn_probs_ref.py.  The maps come from a saving forward (sgl_attention_probs reads q, k and
    the lse from `saved`), so the memory need is that of a training forward."""
    B, H = 128, 16
    m = _model(pkg, "bf16").eval()
    maps = B * H * N * N * 4
    need = _need_or_skip(m, B, True, False, maps + maps // 16 + B * 3 * RES * RES * 4)
    assert maps > 2 ** 32
    rep = _Report(f"output_attentions bf16 B={B}")
    x = _pixels(B, seed=4)
    with torch.no_grad():
        big = m(pixel_values=x, output_attentions=True)
        att, pool = big.attentions[0], big.pooling_attention
        del big
        assert att.shape == (B, H, N, N) and att.dtype == torch.float32
        for lo, hi, _ in _chunks(B):
            ref = m(pixel_values=x[lo:hi], output_attentions=True)
            assert torch.equal(att[lo:hi], ref.attentions[0]), f"attention maps of images {lo}..{hi - 1}"
            assert torch.equal(pool[lo:hi], ref.pooling_attention), f"pooling attention of images {lo}..{hi - 1}"
            del ref
        # four slabs in float64: first, the one that holds byte 2^32 of the output, one mid-range, last
        slab = N * N * 4
        worst = 0.0
        for z in (0, 2 ** 32 // slab, 1000, B * H - 1):
            b, h = divmod(z, H)
            lo = min(b // CHUNK * CHUNK, B - CHUNK)
            q, k, lse, again = _block0_operands(pkg, hiplib, m, x[lo:lo + CHUNK])
            assert torch.equal(again, att[lo:lo + CHUNK]), "the rebuilt q, k, lse are not the operands the model used"
            i = b - lo
            p, bound = apr.probs_ref(q[i:i + 1, h:h + 1, :, :DH], k[i:i + 1, h:h + 1, :, :DH], lse[i:i + 1, h:h + 1], apr.BF16)
            r = apr.worst_ratio(att[b:b + 1, h:h + 1], p, bound)
            assert r <= 1.0, f"attention map (image {b}, head {h}) is {r:.3g} x its float64 bound"
            worst = max(worst, r)
            del q, k, lse, again
    rep.done(f"(computed need {need / 2**30:.1f} GiB; worst slab error / float64 bound {worst:.3f})")
    del att, pool, x, m
    torch.cuda.empty_cache()


DH, DP = 72, 80


def _block0_operands(pkg, lib, m, x8):
    """q, k head-major [8][H][N][80] bf16 and lse [8][H][N] of block 0 for 8 images, rebuilt through the single-kernel entry
    points from the embedding output of a package call on those images: LayerNorm-1 into bf16, the QKV GEMM with its
    head-major scatter on the bf16 cast of the fused weight, the attention forward for the lse.  These are the kernels, at
    the tile dispatch (5832 tokens), that the model ran, so the operands are the model's bit for bit; the caller checks
    that through sgl_op_attn_probs, whose output is returned as the fourth value."""
    H = 16
    cfg = pkg.get_config(CFG)
    sd = {n: t.cuda() for n, t in pkg.weights.seeded_state_dict(cfg, seed=3).items() if n.startswith("encoder.layers.0.")}
    pre = "encoder.layers.0."
    h0 = m(pixel_values=x8, output_hidden_states=True).hidden_states[0].contiguous()
    M = x8.shape[0] * N
    s = torch.cuda.current_stream().cuda_stream
    ok = lambda st: _ok(st)
    h1 = torch.empty(M, D, device="cuda", dtype=torch.bfloat16)
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    ok(lib.sgl_op_layernorm_fwd(h0.data_ptr(), sd[pre + "layer_norm1.weight"].data_ptr(),
                                sd[pre + "layer_norm1.bias"].data_ptr(), h1.data_ptr(), 1, mean.data_ptr(), rstd.data_ptr(),
                                M, D, cfg.layer_norm_eps, s))
    names = ("q_proj", "k_proj", "v_proj")
    w = torch.cat([sd[pre + f"self_attn.{n}.weight"] for n in names]).to(torch.bfloat16).contiguous()
    bias = torch.cat([sd[pre + f"self_attn.{n}.bias"] for n in names]).float().contiguous()
    qkv = torch.empty(3, x8.shape[0], H, N, DP, device="cuda", dtype=torch.bfloat16)
    ok(lib.sgl_op_gemm_nt(1, h1.data_ptr(), D, w.data_ptr(), D, M, 3 * D, D, 3, qkv.data_ptr(), 0, None, 0, bias.data_ptr(),
                          None, 0, None, 0, None, 1, N, H, DH, DP, x8.shape[0], s))
    o = torch.empty(M, D, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(x8.shape[0], H, N, device="cuda")
    ok(lib.sgl_op_attn_fwd(1, qkv[0].data_ptr(), qkv[1].data_ptr(), qkv[2].data_ptr(), o.data_ptr(), lse.data_ptr(),
                           x8.shape[0], H, N, DH, DP, 0, s))
    again = torch.empty(x8.shape[0], H, N, N, device="cuda")
    ok(lib.sgl_op_attn_probs(1, qkv[0].data_ptr(), qkv[1].data_ptr(), lse.data_ptr(), again.data_ptr(), x8.shape[0], H, N, DH,
                             DP, 0, s))
    torch.cuda.synchronize()
    return qkv[0], qkv[1], lse, again


def _ok(st):
    assert st == 0, f"C ABI status {st}"
