"""GPU: sgl_op_preprocess_bwd, the adjoint of Resize(S, antialias=True) -> [MixUp] -> Normalize with respect to a float
source, through the C ABI and up to `x_src.grad`.

The discipline of tests/test_kernel_edges_aux_gpu.py: every element of d_src is held to its own derived bound against
the float64 reference of tests/preprocess_bwd_ref.py (asserted on the CPU in tests/test_preprocess_bwd_host.py), the
output sits between sentinel guard rows with a NaN body, each case is named after the branch it is there for, and every
case prints its worst err/bound as a RATIO line before it asserts.
"""
import pytest
import torch

import kernel_ref as kr
import preprocess_bwd_ref as pb
from test_input_grad_gpu import build
from test_kernel_edges_aux_gpu import BAD_SHAPE, NULL, UNSUPPORTED, WORKSPACE, untouched, within
from test_kernel_edges_gpu import DEV, Guarded, P, lib, ok, stream  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu

# name, (Hs, Ws), S
BRANCHES = [
    ("identity_shortcut", (42, 42), 42),
    ("one_axis_identity", (42, 97), 42),
    ("downscale_nonint", (97, 131), 42),
    ("upscale", (30, 30), 42),
    ("ratio16", (224, 224), 14),
    ("upscale16_long_gather", (7, 9), 112),
    ("odd_sizes", (50, 61), 45),
]
MIX_IDS = ["nomix" if m is None else f"mix_lam{lam}" for m, lam in pb.MIXES]


def scratch_for(lib, B, Hs, Ws, S):
    n = lib.sgl_op_preprocess_bwd_scratch_bytes(B, Hs, Ws, S)
    return (torch.empty(n, device=DEV, dtype=torch.uint8) if n else None), n


def run_bwd(lib, G_d, Hs, Ws, S, std, mix_d, lam, out):
    B = G_d.shape[0]
    scratch, n = scratch_for(lib, B, Hs, Ws, S)
    st = lib.sgl_op_preprocess_bwd(P(G_d), B, Hs, Ws, S, std, P(mix_d), lam, out.ptr, P(scratch), n, stream())
    torch.cuda.synchronize()                             # scratch stays alive until the kernels have run
    return st


def mix_tensor(mix):
    return None if mix is None else torch.tensor(mix, dtype=torch.int32)


@pytest.mark.parametrize("std", [0.5, 0.25])
@pytest.mark.parametrize("mix,lam", pb.MIXES, ids=MIX_IDS)
@pytest.mark.parametrize("geom", BRANCHES, ids=lambda g: g[0])
def test_preprocess_bwd_branches(lib, geom, mix, lam, std):
    name, (Hs, Ws), S = geom
    B = 3
    G = pb.grad_input(B, S, seed=len(name) + Hs)
    out = Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
    G_d, mix_d = G.to(DEV), None if mix is None else mix_tensor(mix).to(DEV)
    ok(run_bwd(lib, G_d, Hs, Ws, S, std, mix_d, lam, out))
    what = f"preprocess_bwd {name} {MIX_IDS[pb.MIXES.index((mix, lam))]} std{std}"
    out.check(what)
    ref, bound = pb.preprocess_bwd_ref(G, Hs, Ws, S, std, mix, lam)
    within(out.got().view(B, 3, Hs, Ws), ref, bound, what)


def test_preprocess_bwd_grid_stride(lib):
    """2 x 3 x 1024 x 768 = 4 718 592 source elements, nine times the 2048 x 256 threads of the capped grid (and more than
    the forward's 16384 x 256): the grid-stride loop's later trips."""
    B, Hs, Ws, S = 2, 1024, 768, 64
    assert B * 3 * Hs * Ws > 16384 * 256
    G = pb.grad_input(B, S, seed=12)
    out = Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
    G_d = G.to(DEV)
    ok(run_bwd(lib, G_d, Hs, Ws, S, 0.5, None, 1.0, out))
    out.check("preprocess_bwd grid-stride")
    ref, bound = pb.preprocess_bwd_ref(G, Hs, Ws, S, 0.5, None, 1.0)
    within(out.got().view(B, 3, Hs, Ws), ref, bound, "preprocess_bwd grid-stride")


@pytest.mark.parametrize("geom", [BRANCHES[2], BRANCHES[5], BRANCHES[0]], ids=lambda g: g[0])
def test_preprocess_bwd_is_bitwise_reproducible(lib, geom):
    name, (Hs, Ws), S = geom
    B = 3
    G_d = pb.grad_input(B, S, seed=3).to(DEV)
    mix_d = mix_tensor([1, 1, 0]).to(DEV)
    a, b = Guarded(B * 3 * Hs, Ws, Ws, torch.float32), Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
    ok(run_bwd(lib, G_d, Hs, Ws, S, 0.5, mix_d, 0.3, a))
    ok(run_bwd(lib, G_d, Hs, Ws, S, 0.5, mix_d, 0.3, b))
    a.check(name), b.check(name)
    assert torch.equal(a.got(), b.got())


def test_preprocess_bwd_refusals_write_nothing(lib):
    B, Hs, Ws, S = 2, 224, 100, 14
    G_d = pb.grad_input(B, S, seed=4).to(DEV)
    out = Guarded(B * 3 * 225, 225, 225, torch.float32)             # large enough for every shape tried below
    scratch, n = scratch_for(lib, B, 225, 225, S)

    def call(g=G_d, Bn=B, Hs_=Hs, Ws_=Ws, S_=S, std=0.5, dst=out.ptr, sc=scratch, nb=n):
        return lib.sgl_op_preprocess_bwd(P(g) if g is not None else None, Bn, Hs_, Ws_, S_, std, None, 1.0, dst, P(sc), nb,
                                         stream())
    assert call(Hs_=225) == UNSUPPORTED and call(Ws_=225) == UNSUPPORTED        # 225 / 14 = 16.07
    assert call(std=0.0) == BAD_SHAPE
    assert call(Bn=0) == BAD_SHAPE and call(Hs_=0) == BAD_SHAPE and call(Ws_=0) == BAD_SHAPE and call(S_=0) == BAD_SHAPE
    assert call(g=None) == NULL and call(dst=None) == NULL and call(sc=None) == NULL
    need = lib.sgl_op_preprocess_bwd_scratch_bytes(B, Hs, Ws, S)
    assert call(nb=need - 1) == WORKSPACE and call(nb=0) == WORKSPACE
    torch.cuda.synchronize()
    untouched(out, "preprocess_bwd refusals")


# ---- autograd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32out", "bf16out"])
@pytest.mark.parametrize("mix,lam", [pb.MIXES[0], pb.MIXES[2]], ids=["nomix", "mix_lam0.3"])
def test_resize_normalize_autograd(pkg, lib, mix, lam, out_dtype):
    pp = pkg.preprocess
    B, Hs, Ws, S = 3, 50, 61, 45
    src = kr.image_source(B, Hs, Ws, False, seed=21)
    mix_d = None if mix is None else mix_tensor(mix).to(DEV)
    x = src.to(DEV).requires_grad_(True)
    y = pp.resize_normalize(x, S, 0.5, 0.25, mix_d, lam, dtype=out_dtype)
    with torch.no_grad():
        y0 = pp.resize_normalize(x, S, 0.5, 0.25, mix_d, lam, dtype=out_dtype)
    assert y.requires_grad and y.grad_fn is not None and not y0.requires_grad
    assert torch.equal(y.detach(), y0) and y.dtype == out_dtype
    assert torch.equal(y0, pp.resize_normalize(src.to(DEV), S, 0.5, 0.25, mix_d, lam, dtype=out_dtype))
    G = pb.grad_input(B, S, seed=22).to(out_dtype)
    y.backward(G.to(DEV))
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    vjp = pp.resize_normalize_backward(G.to(DEV), (Hs, Ws), mix_d, lam, std=0.25)
    assert vjp.dtype == torch.float32 and torch.equal(x.grad, vjp)
    ref, bound = pb.preprocess_bwd_ref(G.float(), Hs, Ws, S, 0.25, mix, lam)
    within(x.grad, ref, bound, f"autograd x.grad mix={mix} {out_dtype}")


@pytest.mark.parametrize("kind", ["fp16", "bf16", "channels_last", "strided"])
def test_resize_normalize_autograd_source_layouts(pkg, lib, kind):
    """The gradient comes back in the source's dtype and shape; a 16-bit source gets the fp32 gradient rounded once."""
    pp = pkg.preprocess
    B, Hs, Ws, S = 2, 30, 37, 42
    src = kr.image_source(B, Hs + 2, Ws, False, seed=23).to(DEV)
    if kind in ("fp16", "bf16"):
        x = src[:, :, :Hs].to(torch.float16 if kind == "fp16" else torch.bfloat16)
    elif kind == "channels_last":
        x = src[:, :, :Hs].contiguous(memory_format=torch.channels_last)
    else:
        x = src[:, :, 1:Hs + 1]                            # a non-contiguous view
        assert not x.is_contiguous()
    x = x.detach().requires_grad_(True)
    y = pp.resize_normalize(x, S)
    assert torch.equal(y.detach(), pp.resize_normalize(x.detach(), S))
    G = pb.grad_input(B, S, seed=24).to(DEV)
    y.backward(G)
    want = pp.resize_normalize_backward(G, (Hs, Ws))
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    assert torch.equal(x.grad, want.to(x.dtype))


def test_backward_for_a_uint8_source_is_the_float_path_on_bytes_over_255(pkg, lib):
    pp = pkg.preprocess
    B, Hs, Ws, S = 2, 40, 33, 32
    u8 = kr.image_source(B, Hs, Ws, True, seed=25).to(DEV)                     # NHWC bytes
    G = pb.grad_input(B, S, seed=26).to(DEV)
    y_u8 = pp.resize_normalize(u8, S)
    assert not y_u8.requires_grad
    xf = (u8.permute(0, 3, 1, 2).float() / 255.0).requires_grad_(True)
    pp.resize_normalize(xf, S).backward(G)
    assert torch.equal(pp.resize_normalize_backward(G, (Hs, Ws)), xf.grad)


# ---- end to end --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_source_gradient_through_the_encoder(pkg, lib, mode):
    """x_src -> resize_normalize -> model(pixel_values=) -> loss on pooler_output.  d_pixels itself is pinned to HF by
    tests/test_input_grad_gpu.py, so the chain rule is what is left to check: x_src.grad is bitwise the VJP of p.grad."""
    pp = pkg.preprocess
    model = build(pkg, "tiny", 3, mode).eval().requires_grad_(False)
    src = kr.image_source(2, 50, 61, False, seed=27).to(DEV)
    w = None

    def loss_of(out):
        nonlocal w
        f = out.pooler_output.float()
        if w is None:
            w = torch.cos(torch.arange(f.numel(), dtype=torch.float32, device=DEV) * 0.37 + 0.11).reshape(f.shape)
        return (f * w).sum()

    x = src.clone().requires_grad_(True)
    out_a = model(pixel_values=pp.resize_normalize(x, 32))
    loss = loss_of(out_a)
    loss.backward()
    p = pp.resize_normalize(src, 32).requires_grad_(True)
    out_b = model(pixel_values=p)
    loss_of(out_b).backward()
    assert torch.equal(out_a.pooler_output, out_b.pooler_output)              # asking for the source gradient moves nothing
    assert torch.equal(out_a.last_hidden_state, out_b.last_hidden_state)
    assert x.grad is not None and x.grad.shape == src.shape and x.grad.abs().max().item() > 0
    assert torch.equal(x.grad, pp.resize_normalize_backward(p.grad, (50, 61)))
    if mode == "fp32":
        x_adv = (src + 0.01 * x.grad.sign()).detach()                         # one FGSM step on the SOURCE raises the loss
        with torch.no_grad():
            adv = loss_of(model(pixel_values=pp.resize_normalize(x_adv, 32))).item()
        print(f"[source FGSM/fp32] loss {loss.item():.6f} -> {adv:.6f}")
        assert adv > loss.item()


# ---- GpuTransform and the refusals ---------------------------------------------------------------------------------
def test_gpu_transform_is_differentiable_in_its_plain_branch(pkg, lib):
    pp = pkg.preprocess
    src = kr.image_source(2, 30, 37, False, seed=28).to(DEV)
    G = pb.grad_input(2, 42, seed=29).to(DEV)
    mod = pp.GpuTransform(42, data_augmentation=True).to(DEV).eval()          # eval: the plain branch
    x = src.clone().requires_grad_(True)
    y = mod(x)
    assert torch.equal(y.detach(), pp.resize_normalize(src, 42))
    y.backward(G)
    assert torch.equal(x.grad, pp.resize_normalize_backward(G, (30, 37)))
    with torch.no_grad():
        y2 = mod(x)
    assert not y2.requires_grad and y2.grad_fn is None
    mod.train()                                                                # augmentation without a grad-requiring source
    assert not mod(src).requires_grad
    with torch.no_grad():
        assert not mod(x).requires_grad                                        # and under no_grad nothing is refused


def test_transforms_without_a_backward_refuse_a_grad_requiring_source(pkg, lib):
    pp = pkg.preprocess
    cfg = pkg.get_config("tiny")
    src = kr.image_source(2, 40, 40, False, seed=30).to(DEV)
    x = src.clone().requires_grad_(True)
    params = pp.sample_augmentation(2, torch.Generator().manual_seed(1))
    calls = {
        "to_patch_operand": lambda t: pp.to_patch_operand(t, cfg, size=32),
        "augment_resize_normalize": lambda t: pp.augment_resize_normalize(t, 32, params),
        "augment_to_patch_operand": lambda t: pp.augment_to_patch_operand(t, cfg, params, size=32),
        "GpuTransform(train, augmentation)": pp.GpuTransform(32, data_augmentation=True).to(DEV).train(),
    }
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match="differentia") as e:
            fn(x)
        assert "resize_normalize" in str(e.value) and "pixel_values=" in str(e.value), name
        fn(src)                                                                # today's path: no gradient asked, no refusal
        with torch.no_grad():
            fn(x)
    with pytest.raises(RuntimeError, match="CUDA tensors only"):               # the is_cuda check stays first
        pp.to_patch_operand(x.detach().cpu().requires_grad_(True), cfg, size=32)
