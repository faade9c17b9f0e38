"""CPU (no GPU): the reference of the augmenting transform's adjoint (tests/aug_bwd_ref.py) and the C ABI's refusals.

* the float64 restatement's forward equals oracle.preprocess_oracle.augment_transform to fp32 rounding;
* torch.autograd on it follows the conventions sgl_op_preprocess_aug_bwd documents where the transform is not
  differentiable (clamp bounds inclusive, max / min ties to the lowest channel, the white pixel under a hue shift);
* every case tests/test_aug_bwd_gpu.py runs keeps its share of pixels within DELTA of a kink under KINK_SHARE (same seeds);
* the geometry bound holds the fp32 restatement with room to spare;
* sgl_op_preprocess_aug_bwd / sgl_op_preprocess_aug_bwd_scratch_bytes exist and every documented argument error returns
  its code before the first HIP call (dummy pointers, no launch: the method of tests/test_abi_aux_host.py);
* `differentiable` defaults to False on both Python entry points.
"""
import inspect

import pytest
import torch

import aug_bwd_ref as ar
import kernel_ref as kr
import preprocess_bwd_ref as pb

OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE, NULL = 0, -1, -2, -3, -5
D = 0x7F0000001000          # a 16-byte aligned dummy device pointer, never dereferenced


@pytest.mark.parametrize("u8", [False, True], ids=["f32src", "u8src"])
def test_float64_forward_equals_the_oracle(u8):
    po = ar._oracle()
    src, S, recs = ar.everything_case(u8)
    recs = recs + [ar.record(False, 5.0, ar.PARAM_SETS[2], [0, 1, 2, 3])]
    src = torch.cat([src, src[:1]])
    want = po.augment_transform(src, S, recs)
    got, _ = ar.forward(ar.as_float(src, torch.float64), S, recs)
    err = (got - want.double()).abs().max().item()
    print(f"FWD everything u8={u8}: max|restatement - oracle| {err:.3e}")
    assert err <= 5e-5       # fp32 resize + fp32 chain of Lipschitz constant <= 7 * 1.5 * 1.5 * 1.4 behind 1 / std = 2
    for n in range(3):
        src, S, recs = ar.colour_case(n)
        got, _ = ar.forward(src.double(), S, recs)
        err = (got - po.augment_transform(src, S, recs).double()).abs().max().item()
        print(f"FWD colour set {n}: {err:.3e}")
        assert err <= 5e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_autograd_conventions(dtype):
    x = torch.tensor([0.0, 1.0, 0.5, -0.1, 1.1], dtype=dtype, requires_grad=True)
    x.clamp(0, 1).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]                     # inclusive at both bounds
    a = torch.tensor([1.0, 1.0, 0.25], dtype=dtype, requires_grad=True)
    torch.max(a.view(3, 1), dim=0).values.sum().backward()
    assert a.grad.tolist() == [1.0, 0.0, 0.0]
    b = torch.tensor([0.5, 0.0, 0.0], dtype=dtype, requires_grad=True)
    torch.min(b.view(3, 1), dim=0).values.sum().backward()
    assert b.grad.tolist() == [0.0, 1.0, 0.0]
    # a white pixel, hue shift 0.2, cotangent (1, 2, 3): (6, 0, 0)
    w = torch.ones(3, 1, 1, dtype=dtype, requires_grad=True)
    flag = torch.zeros(1, 1, dtype=torch.bool)
    out = ar._hue(w, 0.2, flag)
    assert out.flatten().tolist() == [1.0, 1.0, 1.0] and not bool(flag.any())
    out.backward(torch.tensor([1.0, 2.0, 3.0], dtype=dtype).view(3, 1, 1))
    assert w.grad.flatten().tolist() == [6.0, 0.0, 0.0]
    # where() differentiates the selected branch only; floor and % contribute nothing
    z = torch.tensor([0.3, 1.7], dtype=dtype, requires_grad=True)
    (torch.where(z > 1, z * 2, z * 3) + torch.floor(z) + (z % 1.0)).sum().backward()
    assert z.grad.tolist() == [4.0, 3.0]


def _cases():
    for n in range(3):
        yield f"colour{n}", ar.colour_case(n)
    for u8 in (False, True):
        yield f"everything_u8{int(u8)}", ar.everything_case(u8)


def test_kink_share_of_every_gpu_case():
    for name, (src, S, recs) in _cases():
        _, share = ar.masked_cotangent(src, S, recs, seed=1)
        print(f"KINK {name}: worst {share.max().item():.4f} mean {share.mean().item():.4f}")
        assert share.max().item() <= ar.KINK_SHARE, name


def test_masked_pixels_cannot_reach_the_gradient():
    """The cotangent of a flagged pixel is zero, so changing it changes nothing: the VJP's colour part is per pixel."""
    src, S, recs = ar.colour_case(0)
    cot, _ = ar.masked_cotangent(src, S, recs, seed=2)
    ref = ar.vjp(src, S, recs, cot)
    m32 = ar.metrics(ar.vjp(src, S, recs, cot, dtype=torch.float32), ref)
    print(f"FP32 colour set 0: worst max-ratio {m32[0].max().item():.3e} rel-L2 {m32[1].max().item():.3e}")
    assert m32[0].max().item() < 1e-5 and m32[1].max().item() < 1e-5
    assert bool(torch.isfinite(ref).all()) and ref.abs().max().item() > 0


@pytest.mark.parametrize("geom", ar.GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}to{g[1]}")
def test_geometry_reference_and_bound(geom):
    """geometry_ref equals autograd on the float64 restatement up to the difference of the two float64 filters (the
    oracle's weights are rounded to fp32), and its bound holds the fp32 restatement's gradient."""
    (Hs, Ws), S = geom
    recs = ar.GEOMETRY_RECORDS
    G = pb.grad_input(3, S, seed=Hs + S)
    ref, bound = ar.geometry_ref(G, Hs, Ws, S, 0.5, recs)
    src = ar.uniform_source(3, Hs, Ws, False, seed=3)
    a64 = ar.vjp(src, S, recs, G)
    assert (ref - a64).abs().max().item() <= 4e-6 * ref.abs().max().item()
    assert bool((bound > 0).all())
    r = kr.worst_ratio(ar.vjp(src, S, recs, G, dtype=torch.float32), ref, bound)
    print(f"RATIO geometry {Hs}x{Ws}->{S}: torch-fp32 {r:.4f}")
    assert r <= 1.0


def test_symbols_exist_and_argument_errors_return_before_any_launch(pkg, hiplib):
    lib = hiplib
    declared = pkg.lib.declared_symbols()
    for s in ("sgl_op_preprocess_aug_bwd", "sgl_op_preprocess_aug_bwd_scratch_bytes"):
        assert s in declared, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.sgl_abi_version() == 3                               # new symbols only
    B, Hs, Ws, S = 2, 30, 50, 42
    need = lib.sgl_op_preprocess_aug_bwd_scratch_bytes(B, Hs, Ws, S)
    blocks = (S * S + 255) // 256
    assert need == lib.sgl_op_preprocess_bwd_scratch_bytes(B, Hs, Ws, S) + 4 * (2 * B + B * blocks + 2 * B * 3 * S * S)
    assert lib.sgl_op_preprocess_aug_bwd_scratch_bytes(0, Hs, Ws, S) == 0
    assert lib.sgl_op_preprocess_aug_bwd_scratch_bytes(B, Hs, Ws, 0) == 0

    def call(d_out=D, src=D, u8=0, Bn=B, Hs_=Hs, Ws_=Ws, S_=S, std=0.5, aug=D, d_src=D, scratch=D, nbytes=need):
        return lib.sgl_op_preprocess_aug_bwd(d_out, src, u8, Bn, Hs_, Ws_, S_, std, aug, d_src, scratch, nbytes, None)
    for u8 in (0, 1):
        for name in ("d_out", "src", "aug", "d_src", "scratch"):
            assert call(u8=u8, **{name: None}) == NULL, name
        assert call(u8=u8, d_out=None, Bn=0) == NULL                # pointers are checked first
        assert call(u8=u8, std=0.0) == BAD_SHAPE
        for over in (dict(Bn=0), dict(Hs_=0), dict(Ws_=0), dict(S_=0), dict(Bn=-1)):
            assert call(u8=u8, **over) == BAD_SHAPE, over
        assert call(u8=u8, Hs_=673) == UNSUPPORTED                  # 673 > 16 * 42
        assert call(u8=u8, Ws_=225, S_=14) == UNSUPPORTED           # 225 > 16 * 14
        assert call(u8=u8, nbytes=need - 1) == WORKSPACE and call(u8=u8, nbytes=0) == WORKSPACE
        assert call(u8=u8, Hs_=672, nbytes=0) == WORKSPACE          # exactly 16x is admitted: the next check answers


def test_differentiable_is_opt_in(pkg):
    pp = pkg.preprocess
    for fn in (pp.augment_resize_normalize, pp.GpuTransform):
        assert inspect.signature(fn).parameters["differentiable"].default is False
    assert "differentiable" not in inspect.signature(pp.augment_to_patch_operand).parameters
    assert list(inspect.signature(pp.augment_resize_normalize_backward).parameters) == ["grad_out", "images", "params", "std"]
