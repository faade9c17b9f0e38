"""GPU: sgl_op_preprocess_aug_bwd, the adjoint of the augmenting transform resize -> flip -> rotation -> colour jitter ->
normalise with respect to its source, through the C ABI and up to `x_src.grad`.

The discipline of tests/test_preprocess_bwd_gpu.py: outputs sit between sentinel guard rows with a NaN body, every case
prints its worst ratio before it asserts.  Geometry alone is linear and held element by element to the derived bound of
tests/aug_bwd_ref.py.  With colour operators the bound cannot be derived (the hue step divides by max - min), so it is
measured per image against the reference's own fp32 arithmetic: the float64 restatement under torch.autograd is the
reference, the same restatement in fp32 on the CPU the yardstick, and the kernel has to stay within MARGIN = 8 times the
yardstick's error (never below 32 * 2^-24) in max|e| / max|ref| and in relative L2.  The cotangent is zero on pixels within
1e-4 of a kink (tests/test_aug_bwd_host.py holds their share under 3 %), so every element of d_src is compared.
"""
import pytest
import torch

import aug_bwd_ref as ar
import kernel_ref as kr
import preprocess_bwd_ref as pb
from test_input_grad_gpu import build
from test_kernel_edges_aux_gpu import BAD_SHAPE, NULL, UNSUPPORTED, WORKSPACE, untouched, within
from test_kernel_edges_gpu import DEV, Guarded, P, lib, ok, stream  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu


def run_bwd(pkg, lib, G_d, src_d, recs, S, std, out):
    u8 = src_d.dtype == torch.uint8
    B = src_d.shape[0]
    Hs, Ws = (src_d.shape[1], src_d.shape[2]) if u8 else (src_d.shape[2], src_d.shape[3])
    tab = pkg.preprocess.augment_table(recs, DEV)
    n = lib.sgl_op_preprocess_aug_bwd_scratch_bytes(B, Hs, Ws, S)
    scratch = torch.empty(n, device=DEV, dtype=torch.uint8)
    st = lib.sgl_op_preprocess_aug_bwd(P(G_d), P(src_d), int(u8), B, Hs, Ws, S, std, P(tab), out.ptr, P(scratch), n, stream())
    torch.cuda.synchronize()                             # scratch and the table stay alive until the kernels have run
    return st


def hw_of(src):
    return (src.shape[1], src.shape[2]) if src.dtype == torch.uint8 else (src.shape[2], src.shape[3])


def check_colour(what, got, src, S, recs, cot, std=0.5):
    """Per image, both metrics, against MARGIN x the fp32 restatement's error (floor FLOOR); returns the worst ratio."""
    ref = ar.vjp(src, S, recs, cot, std)
    b_inf, b_l2 = ar.colour_bound(src, S, recs, cot, ref, std)
    m_inf, m_l2 = ar.metrics(got.detach().cpu(), ref)
    r_inf, r_l2 = (m_inf / b_inf), (m_l2 / b_l2)
    worst = max(r_inf.max().item(), r_l2.max().item())
    print(f"RATIO {what}: max {r_inf.max().item():.4f} (image {r_inf.argmax().item()}) "
          f"l2 {r_l2.max().item():.4f} (image {r_l2.argmax().item()}) | kernel max|e|/max|ref| {m_inf.max().item():.3e} "
          f"rel-L2 {m_l2.max().item():.3e} | fp32 restatement {(b_inf / ar.MARGIN).max().item():.3e} "
          f"{(b_l2 / ar.MARGIN).max().item():.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert worst <= 1.0, f"{what}: {worst:.3f} x the bound"
    return worst


# ---- 1. geometry alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32src", "u8src"])
@pytest.mark.parametrize("geom", ar.GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}to{g[1]}")
def test_geometry_alone(pkg, lib, geom, u8):
    """flip only; +5 degrees with flip; -30 degrees (the zero corners): antialiased downscale, upscale, copy shortcut."""
    (Hs, Ws), S = geom
    recs, B = ar.GEOMETRY_RECORDS, 3
    G = pb.grad_input(B, S, seed=Hs + S)
    src = ar.uniform_source(B, Hs, Ws, u8, seed=7)
    for std in (0.5, 0.25):
        out = Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
        ok(run_bwd(pkg, lib, G.to(DEV), src.to(DEV), recs, S, std, out))
        what = f"aug_bwd geometry {Hs}x{Ws}->{S} u8={int(u8)} std{std}"
        out.check(what)
        ref, bound = ar.geometry_ref(G, Hs, Ws, S, std, recs)
        within(out.got().view(B, 3, Hs, Ws), ref, bound, what)


# ---- 2. colour alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2], ids=lambda n: "b%g_c%g_s%g_h%g" % ar.PARAM_SETS[n])
def test_colour_alone(pkg, lib, n):
    """Hs = Ws = S = 16, no flip, no rotation: the 24 orders and each operator alone, one image each."""
    src, S, recs = ar.colour_case(n)
    B = len(recs)
    cot, share = ar.masked_cotangent(src, S, recs, seed=40 + n)
    assert share.max().item() <= ar.KINK_SHARE
    out = Guarded(B * 3 * S, S, S, torch.float32)
    ok(run_bwd(pkg, lib, cot.to(DEV), src.to(DEV), recs, S, 0.5, out))
    out.check(f"aug_bwd colour {n}")
    check_colour(f"aug_bwd colour set {n}", out.got().view(B, 3, S, S), src, S, recs, cot)


# ---- 3. everything -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32src", "u8src"])
def test_everything(pkg, lib, u8):
    src, S, recs = ar.everything_case(u8)
    B, (Hs, Ws) = len(recs), hw_of(src)
    cot, share = ar.masked_cotangent(src, S, recs, seed=50 + int(u8))
    assert share.max().item() <= ar.KINK_SHARE
    out = Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
    ok(run_bwd(pkg, lib, cot.to(DEV), src.to(DEV), recs, S, 0.5, out))
    out.check(f"aug_bwd everything u8={u8}")
    check_colour(f"aug_bwd everything u8={int(u8)}", out.got().view(B, 3, Hs, Ws), src, S, recs, cot)


# ---- 4. more source elements than one pass of the capped grid ------------------------------------------------------------
def test_grid_stride_of_the_resize_adjoint(pkg, lib):
    """The colour and rotation kernels launch one block per 256 pixels and never loop; the resize adjoint caps its grid at
    2048 blocks: 2 x 3 x 300 x 300 = 540 000 source elements is the smallest square batch of two past 2048 x 256."""
    (Hs, Ws), S, B = ar.GRID_CASE
    assert B * 3 * Hs * Ws > 2048 * 256 >= B * 3 * (Hs - 5) * (Ws - 5)
    recs = ar.GEOMETRY_RECORDS[1:]
    G = pb.grad_input(B, S, seed=61)
    src = ar.uniform_source(B, Hs, Ws, False, seed=62)
    out = Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
    ok(run_bwd(pkg, lib, G.to(DEV), src.to(DEV), recs, S, 0.5, out))
    out.check("aug_bwd grid-stride")
    ref, bound = ar.geometry_ref(G, Hs, Ws, S, 0.5, recs)
    within(out.got().view(B, 3, Hs, Ws), ref, bound, "aug_bwd grid-stride")


# ---- 5. reproducibility, refusals ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32src", "u8src"])
def test_two_runs_give_the_same_bits(pkg, lib, u8):
    src, S, recs = ar.everything_case(u8)
    B, (Hs, Ws) = len(recs), hw_of(src)
    G_d, src_d = pb.grad_input(B, S, seed=70).to(DEV), src.to(DEV)
    a, b = Guarded(B * 3 * Hs, Ws, Ws, torch.float32), Guarded(B * 3 * Hs, Ws, Ws, torch.float32)
    ok(run_bwd(pkg, lib, G_d, src_d, recs, S, 0.5, a))
    ok(run_bwd(pkg, lib, G_d, src_d, recs, S, 0.5, b))
    a.check("run 1"), b.check("run 2")
    assert torch.equal(a.got(), b.got())


@pytest.mark.parametrize("u8", [False, True], ids=["f32src", "u8src"])
def test_recomputed_grey_means_have_the_forward_bits(pkg, lib, u8):
    """The backward evaluates the contrast step's grey mean with one thread per pixel and then repeats the forward's sum
    over the stored terms: the B floats behind the resize tables in its scratch are the forward's grey_mean, bit for bit
    (0 for an image without a contrast step).  300 x 300 -> 40: S * S is no multiple of 256 and spans several blocks."""
    B, Hs, Ws, S = 4, 300, 300, 40
    recs = [ar.record(True, 5.0, ar.PARAM_SETS[0], [3, 0, 1, 2]), ar.record(False, 0.0, ar.PARAM_SETS[1], [1, 2, 3, 0]),
            ar.record(False, -30.0, ar.PARAM_SETS[2], None), ar.record(True, 0.0, ar.PARAM_SETS[2], [2, 0, 3, 1])]
    src_d = ar.uniform_source(B, Hs, Ws, u8, seed=71).to(DEV)
    tab = pkg.preprocess.augment_table(recs, DEV)
    fwd, gm = torch.empty(B, 3, S, S, device=DEV), torch.full((B,), float("nan"), device=DEV)
    ok(lib.sgl_op_preprocess_aug(P(src_d), int(u8), B, Hs, Ws, P(fwd), 0, S, 1, 3, 0, 0.5, 0.5, P(tab), P(gm), stream()))
    n = lib.sgl_op_preprocess_aug_bwd_scratch_bytes(B, Hs, Ws, S)
    scratch = torch.empty(n, device=DEV, dtype=torch.uint8)
    d_src = torch.empty(B, 3, Hs, Ws, device=DEV)
    G_d = pb.grad_input(B, S, seed=72).to(DEV)
    ok(lib.sgl_op_preprocess_aug_bwd(P(G_d), P(src_d), int(u8), B, Hs, Ws, S, 0.5, P(tab), P(d_src), P(scratch), n, stream()))
    torch.cuda.synchronize()
    off = lib.sgl_op_preprocess_bwd_scratch_bytes(B, Hs, Ws, S)
    again = scratch[off:off + 4 * B].view(torch.float32)
    print(f"GREY forward {gm.tolist()} backward {again.tolist()}")
    assert gm[2].item() == 0.0 and bool((gm[[0, 1, 3]] > 0).all())
    assert torch.equal(gm, again)


def test_refusals_write_nothing(pkg, lib):
    B, Hs, Ws, S = 2, 224, 100, 14
    G_d = pb.grad_input(B, S, seed=4).to(DEV)
    src_d = ar.uniform_source(B, 225, 225, False, seed=5).to(DEV)            # large enough for every shape tried below
    tab = pkg.preprocess.augment_table(ar.GEOMETRY_RECORDS[:B], DEV)
    out = Guarded(B * 3 * 225, 225, 225, torch.float32)
    n = lib.sgl_op_preprocess_aug_bwd_scratch_bytes(B, 225, 225, S)
    scratch = torch.empty(n, device=DEV, dtype=torch.uint8)

    def call(g=G_d, src=src_d, Bn=B, Hs_=Hs, Ws_=Ws, S_=S, std=0.5, aug=tab, dst=out.ptr, sc=scratch, nb=n):
        return lib.sgl_op_preprocess_aug_bwd(P(g), P(src), 0, Bn, Hs_, Ws_, S_, std, P(aug), dst, P(sc), nb, stream())
    assert call(Hs_=225) == UNSUPPORTED and call(Ws_=225) == UNSUPPORTED        # 225 / 14 = 16.07
    assert call(std=0.0) == BAD_SHAPE
    assert call(Bn=0) == BAD_SHAPE and call(Hs_=0) == BAD_SHAPE and call(Ws_=0) == BAD_SHAPE and call(S_=0) == BAD_SHAPE
    assert call(g=None) == NULL and call(src=None) == NULL and call(aug=None) == NULL
    assert call(dst=None) == NULL and call(sc=None) == NULL
    need = lib.sgl_op_preprocess_aug_bwd_scratch_bytes(B, Hs, Ws, S)
    assert call(nb=need - 1) == WORKSPACE and call(nb=0) == WORKSPACE
    torch.cuda.synchronize()
    untouched(out, "aug_bwd refusals")


# ---- 6. autograd surface -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32out", "bf16out"])
def test_autograd_equals_the_function_and_moves_no_forward_bit(pkg, lib, out_dtype):
    pp = pkg.preprocess
    src, S, recs = ar.everything_case(False)
    B, (Hs, Ws) = len(recs), hw_of(src)
    x = src.to(DEV).requires_grad_(True)
    y = pp.augment_resize_normalize(x, S, recs, 0.5, 0.25, dtype=out_dtype, differentiable=True)
    y0 = pp.augment_resize_normalize(src.to(DEV), S, recs, 0.5, 0.25, dtype=out_dtype)
    assert y.requires_grad and y.grad_fn is not None and not y0.requires_grad
    assert torch.equal(y.detach(), y0) and y.dtype == out_dtype
    with torch.no_grad():
        assert torch.equal(pp.augment_resize_normalize(x, S, recs, 0.5, 0.25, dtype=out_dtype, differentiable=True), y0)
    cot, _ = ar.masked_cotangent(src, S, recs, seed=80)
    cot = cot.to(out_dtype)
    y.backward(cot.to(DEV))
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    vjp = pp.augment_resize_normalize_backward(cot.to(DEV), src.to(DEV), recs, std=0.25)
    assert vjp.dtype == torch.float32 and torch.equal(x.grad, vjp)
    check_colour(f"aug autograd {out_dtype}", x.grad, src, S, recs, cot.float(), std=0.25)
    with pytest.raises(RuntimeError):                                          # once_differentiable: no double backward
        x2 = src.to(DEV).requires_grad_(True)
        y2 = pp.augment_resize_normalize(x2, S, recs, differentiable=True)
        (g2,) = torch.autograd.grad(y2.sum(), x2, create_graph=True)
        g2.sum().backward()


@pytest.mark.parametrize("kind", ["fp32", "fp16", "bf16", "channels_last"])
def test_gradient_arrives_in_the_source_dtype_and_strides(pkg, lib, kind):
    pp = pkg.preprocess
    src, S, recs = ar.everything_case(False)
    src = src.to(DEV)
    if kind in ("fp16", "bf16"):
        x = src.to(torch.float16 if kind == "fp16" else torch.bfloat16)
    elif kind == "channels_last":
        x = src.contiguous(memory_format=torch.channels_last)
    else:
        x = src.clone()
    x = x.detach().requires_grad_(True)
    y = pp.augment_resize_normalize(x, S, recs, differentiable=True)
    assert torch.equal(y.detach(), pp.augment_resize_normalize(x.detach(), S, recs))
    G = pb.grad_input(len(recs), S, seed=81).to(DEV)
    y.backward(G)
    want = pp.augment_resize_normalize_backward(G, x.detach(), recs)
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape and x.grad.stride() == x.stride()
    assert torch.equal(x.grad, want.to(x.dtype))


def test_backward_function_serves_uint8_sources(pkg, lib):
    """uint8 NHWC bytes and the float NCHW tensor bytes / 255 are the same source: the same gradient, bit for bit when the
    float tensor holds fl(byte * fl(1 / 255)), the value the kernel reads."""
    pp = pkg.preprocess
    src, S, recs = ar.everything_case(True)
    u8 = src.to(DEV)
    G = pb.grad_input(len(recs), S, seed=82).to(DEV)
    xf = (u8.permute(0, 3, 1, 2).float() * torch.tensor(1.0 / 255.0, dtype=torch.float32, device=DEV)).contiguous()
    assert not pp.augment_resize_normalize(u8, S, recs, differentiable=True).requires_grad
    a = pp.augment_resize_normalize_backward(G, u8, recs)
    assert a.shape == xf.shape and torch.equal(a, pp.augment_resize_normalize_backward(G, xf, recs))


def test_gpu_transform_differentiable_training_branch(pkg, lib):
    pp = pkg.preprocess
    src = kr.image_source(4, 30, 37, False, seed=83).to(DEV)
    G = pb.grad_input(4, 24, seed=84).to(DEV)
    mod = pp.GpuTransform(24, data_augmentation=True, generator=torch.Generator().manual_seed(9),
                          differentiable=True).to(DEV).train()
    x = src.clone().requires_grad_(True)
    y = mod(x)
    recs = pp.sample_augmentation(4, torch.Generator().manual_seed(9))
    assert y.requires_grad and torch.equal(y.detach(), pp.augment_resize_normalize(src, 24, recs))
    y.backward(G)
    assert torch.equal(x.grad, pp.augment_resize_normalize_backward(G, src, recs))
    mod.eval()                                                                  # eval: the plain branch, as before
    x2 = src.clone().requires_grad_(True)
    y2 = mod(x2)
    assert torch.equal(y2.detach(), pp.resize_normalize(src, 24))
    y2.backward(G)
    assert torch.equal(x2.grad, pp.resize_normalize_backward(G, (30, 37)))


def test_default_calls_still_refuse(pkg, lib):
    pp = pkg.preprocess
    cfg = pkg.get_config("tiny")
    src = kr.image_source(2, 40, 40, False, seed=85).to(DEV)
    x = src.clone().requires_grad_(True)
    recs = pp.sample_augmentation(2, torch.Generator().manual_seed(1))
    calls = {
        "augment_resize_normalize": lambda t: pp.augment_resize_normalize(t, 32, recs),
        "augment_resize_normalize(differentiable=False)": lambda t: pp.augment_resize_normalize(t, 32, recs, differentiable=False),
        "augment_to_patch_operand": lambda t: pp.augment_to_patch_operand(t, cfg, recs, size=32),
        "GpuTransform(train, augmentation)": pp.GpuTransform(32, data_augmentation=True).to(DEV).train(),
    }
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match="differentia") as e:
            fn(x)
        assert "resize_normalize" in str(e.value) and "pixel_values=" in str(e.value), name
        fn(src)
    with pytest.raises(TypeError):
        pp.augment_to_patch_operand(x, cfg, recs, size=32, differentiable=True)


def test_source_gradient_through_the_encoder_against_the_cpu_oracle_chain(pkg, oracle, lib):
    """x_src -> augment_resize_normalize(differentiable=True) -> tiny encoder (fp32) -> loss, against the same chain on the
    CPU: the restatement, then oracle/siglip_oracle.py, in float64 (the reference) and in float32 (the yardstick).  Pixels
    within DELTA of a kink are taken out of the graph on every side (their value stays, their cotangent is zero)."""
    pp = pkg.preprocess
    cfg = pkg.get_config("tiny")
    sd = pkg.weights.seeded_state_dict(cfg, seed=3)
    model = build(pkg, "tiny", 3, "fp32").eval().requires_grad_(False)
    S = 32
    recs = [ar.record(True, 5.0, ar.PARAM_SETS[2], [1, 3, 0, 2]), ar.record(False, -4.0, ar.PARAM_SETS[1], [0, 2, 3, 1])]
    src = kr.image_source(2, 50, 61, False, seed=86)
    flag = ar.flags_of(src, S, recs)
    assert flag.double().mean().item() <= ar.KINK_SHARE
    keep = (~flag)[:, None]
    w = None

    def loss_of(f):
        nonlocal w
        if w is None:
            w = torch.cos(torch.arange(f.numel(), dtype=torch.float64) * 0.37 + 0.11).reshape(f.shape)
        return (f * w.to(device=f.device, dtype=f.dtype)).sum()

    def cpu_chain(dtype):
        x = src.to(dtype).clone().requires_grad_(True)         # .to() alone returns src itself for float32
        y, _ = ar.forward(x, S, recs)
        y = torch.where(keep, y, y.detach())
        out = oracle.vision_forward(y, oracle.cast_state_dict(sd, dtype), cfg, False, False)
        loss_of(out["pooler_output"]).backward()
        return x.grad

    ref, f32 = cpu_chain(torch.float64), cpu_chain(torch.float32)
    x = src.to(DEV).requires_grad_(True)
    y = pp.augment_resize_normalize(x, S, recs, differentiable=True)
    y = torch.where(keep.to(DEV), y, y.detach())
    loss_of(model(pixel_values=y).pooler_output.float()).backward()
    m_inf, m_l2 = ar.metrics(x.grad.cpu(), ref)
    y_inf, y_l2 = ar.metrics(f32, ref)
    b_inf, b_l2 = (ar.MARGIN * y_inf).clamp_min(ar.FLOOR), (ar.MARGIN * y_l2).clamp_min(ar.FLOOR)
    worst = max((m_inf / b_inf).max().item(), (m_l2 / b_l2).max().item())
    print(f"RATIO aug end-to-end tiny/fp32: {worst:.4f} | kernel max|e|/max|ref| {m_inf.max().item():.3e} rel-L2 "
          f"{m_l2.max().item():.3e} | fp32 chain {y_inf.max().item():.3e} {y_l2.max().item():.3e}")
    assert ref.abs().max().item() > 0 and worst <= 1.0
