"""CPU (no GPU): the reference of the input transform's adjoint (tests/preprocess_bwd_ref.py) and the C ABI's refusals.

* the float64 reference `Wy^T G Wx` (+ MixUp, 1 / std) built on kernel_ref.aa_axis equals torch's own float64 autograd of
  F.interpolate(bilinear, antialias=True) -> MixUp -> normalise to 1e-12 on unit-variance G, on six geometries with and
  without mix_index = [1, 1, 0] (an image referenced twice, a fixed point, one never referenced);
* fp32 evaluations of the same operation (torch's fp32 CPU backward, and the kernel's weight arithmetic restated in torch
  fp32) stay inside the derived bound with worst ratio <= 0.5, the rule tests/test_kernel_ref_host.py holds fp32 outputs to;
* sgl_op_preprocess_bwd / sgl_op_preprocess_bwd_scratch_bytes exist and every documented argument error returns its code
  before the first HIP call (dummy pointers, no launch: the method of tests/test_abi_aux_host.py).
"""
import pytest
import torch

import kernel_ref as kr
import preprocess_bwd_ref as pb

OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE, NULL = 0, -1, -2, -3, -5
D = 0x7F0000001000          # a 16-byte aligned dummy device pointer, never dereferenced
B = 3
IDS = [f"{hs}x{ws}to{s}" for (hs, ws), s in pb.GEOMETRIES]
MIX_IDS = ["nomix" if m is None else f"mix_lam{lam}" for m, lam in pb.MIXES]


@pytest.mark.parametrize("mix,lam", pb.MIXES, ids=MIX_IDS)
@pytest.mark.parametrize("geom", pb.GEOMETRIES, ids=IDS)
def test_reference_equals_torch_float64_autograd(geom, mix, lam):
    (Hs, Ws), S = geom
    G = pb.grad_input(B, S, seed=Hs + S)
    for std in (0.5, 0.25):
        ref, _ = pb.preprocess_bwd_ref(G, Hs, Ws, S, std, mix, lam)
        want = pb.torch_autograd_f64(G, Hs, Ws, S, std, mix, lam)
        err = (ref - want).abs().max().item()
        print(f"REFERR {Hs}x{Ws}->{S} std {std} mix {mix} lam {lam}: {err:.3e}")
        assert tuple(ref.shape) == (B, 3, Hs, Ws)
        assert err <= 1e-12


@pytest.mark.parametrize("mix,lam", pb.MIXES, ids=MIX_IDS)
@pytest.mark.parametrize("geom", pb.GEOMETRIES + [((42, 42), 42), ((50, 61), 45)], ids=IDS + ["identity", "50x61to45"])
def test_fp32_emulations_stay_inside_half_the_bound(geom, mix, lam):
    """Measured worst ratios (emulation / torch fp32 backward): 0.34 / 0.34 at the copy shortcut with MixUp at lam 0.3,
    where the blend's roundings are all there is; 0.12 / 0.12 at (50, 50) -> 45 and below 0.05 on the other resampling
    geometries (pytest -rP prints every case)."""
    (Hs, Ws), S = geom
    G = pb.grad_input(B, S, seed=Hs + S + 1)
    for std in (0.5, 0.25):
        ref, bound = pb.preprocess_bwd_ref(G, Hs, Ws, S, std, mix, lam)
        assert bool((bound > 0).all())
        emu = pb.emulate_f32(G, Hs, Ws, S, std, mix, lam)
        r_emu = kr.assert_within(emu, ref, bound, f"emulation {geom} {mix} {lam}")
        tf32 = pb.torch_autograd_f64(G, Hs, Ws, S, std, mix, lam, dtype=torch.float32)
        r_t = kr.assert_within(tf32, ref, bound, f"torch fp32 backward {geom} {mix} {lam}")
        print(f"RATIO {Hs}x{Ws}->{S} std {std} mix {mix} lam {lam}: emulation {r_emu:.4f} torch-fp32 {r_t:.4f}")
        assert r_emu <= 0.5 and r_t <= 0.5


def test_bound_catches_a_dropped_boundary_tap():
    """The mutant the exact-membership search is there to prevent: the last covering output of every source column left
    out.  Its weight is small but not zero, and the bound must not absorb it."""
    (Hs, Ws), S = (97, 131), 42
    G = pb.grad_input(B, S, seed=5)
    ref, bound = pb.preprocess_bwd_ref(G, Hs, Ws, S, 0.5, None, 1.0)
    Wy, Wx = pb._axis_f32(S, Hs), pb._axis_f32(S, Ws)
    last = ((Wx > 0) * (torch.arange(S)[:, None] + 1)).argmax(0)      # the last output with a positive weight, per column
    Wx_drop = Wx.clone()
    Wx_drop[last, torch.arange(Ws)] = 0
    mutant = (Wy.t() @ G @ Wx_drop) * 2.0
    assert kr.worst_ratio(mutant, ref, bound) > 100


def test_symbols_exist_and_argument_errors_return_before_any_launch(pkg, hiplib):
    lib = hiplib
    declared = pkg.lib.declared_symbols()
    for s in ("sgl_op_preprocess_bwd", "sgl_op_preprocess_bwd_scratch_bytes"):
        assert s in declared, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.sgl_abi_version() == 3                               # new symbols only
    need = lib.sgl_op_preprocess_bwd_scratch_bytes(2, 30, 50, 42)
    assert need == 2 * 42 * 20 + (30 + 50) * 8                      # two filter tables, two span tables
    assert lib.sgl_op_preprocess_bwd_scratch_bytes(2, 42, 42, 42) == 0      # the copy shortcut needs none

    def call(d_out=D, Bn=2, Hs=30, Ws=50, S=42, std=0.5, mix=None, lam=1.0, d_src=D, scratch=D, nbytes=need):
        return lib.sgl_op_preprocess_bwd(d_out, Bn, Hs, Ws, S, std, mix, lam, d_src, scratch, nbytes, None)
    assert call(d_out=None) == NULL and call(d_src=None) == NULL
    assert call(d_out=None, Bn=0) == NULL                           # pointers are checked first
    assert call(std=0.0) == BAD_SHAPE
    for over in (dict(Bn=0), dict(Hs=0), dict(Ws=0), dict(S=0), dict(Bn=-1)):
        assert call(**over) == BAD_SHAPE, over
    assert call(Hs=673) == UNSUPPORTED                              # 673 > 16 * 42
    assert call(Ws=225, S=14) == UNSUPPORTED                        # 225 > 16 * 14
    assert call(nbytes=need - 1) == WORKSPACE and call(nbytes=0) == WORKSPACE
    assert call(scratch=None) == NULL                               # bytes are needed here
    assert call(Hs=672, nbytes=0) == WORKSPACE                      # exactly 16x is admitted: the next check answers
