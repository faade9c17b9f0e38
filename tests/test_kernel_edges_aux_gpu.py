"""GPU tests of the HIP kernels OUTSIDE the encoder, through the C ABI (``sgl_op_*``): the input pipeline
(csrc/preprocess.hip), the video tail (csrc/video_tail.hip), the depthwise 3x3 (csrc/decoder.hip), the decoder tail
(csrc/decoder_tail.hip) and AdamW (csrc/optimizer.hip).

Same discipline as tests/test_kernel_edges_gpu.py: every output element is held to its own bound against a float64
reference of the same operation on the same rounded inputs (tests/kernel_ref.py; the bounds are asserted against CPU
emulations in tests/test_kernel_ref_host.py), every output sits between sentinel guard rows with a NaN body, and each case
is named after the branch it is there for.  The one place an element may be left out is the hue operator (the reference's
own `excused` mask, at most 1 % of any image; tests/test_kernel_ref_host.py asserts the share on these very inputs).
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import kernel_ref as kr
from kernel_ref import BF16, F16, F32
from test_kernel_edges_gpu import DEV, Guarded, P, gen, lib, ok, randn, stream, tdt_of  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu
OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE, NULL = 0, -1, -2, -3, -5


def flat(n, tdt, prior=None):
    """A guarded 1-D output of n elements (as rows of 4096 when it is long, so the guard bands stay small)."""
    ld = n if n <= 65536 else 4096
    assert n % ld == 0
    return Guarded(n // ld, ld, ld, tdt, prior)


def untouched(gd, what):
    """Guards intact and the NaN body still NaN everywhere: the call wrote nothing."""
    gd.check(what, written=False)
    assert bool(torch.isnan(gd.got().float()).all()), f"{what}: the output was written"


def within(got, ref, bound, what):
    """kernel_ref.assert_within on the reference's device; prints the worst err/bound of the case (pytest -rP shows it:
    the per-kernel worst ratios of DESIGN.md are the maxima of these lines)."""
    r = kr.assert_within(got.detach().to(ref.device), ref, bound, what)
    print(f"RATIO {what.split()[0]} {r:.4f}  {what}")
    return r


# =========================================================================================================
# sgl_op_preprocess
# =========================================================================================================
def preprocess(lib, src, u8, out, dtype, B, Hs, Ws, S, Pp, Kp, patch, mix=None, lam=1.0, mean=0.5, std=0.5):
    return lib.sgl_op_preprocess(P(src), int(u8), B, Hs, Ws, out, dtype, S, Pp, Kp, int(patch), mean, std, P(mix), lam,
                                 stream())


def out_buffer(B, S, Pp, Kp, patch, tdt):
    if patch:
        g = S // Pp
        return Guarded(B * g * g, Kp, Kp, tdt)
    return Guarded(B * 3 * S, S, S, tdt)


# name, (Hs, Ws), S, P, Kp, patch-major, mix lam (None = no MixUp)
PRE_GEOM = [
    ("identity_shortcut", (42, 42), 42, 14, 640, False, None),
    ("one_axis_identity", (42, 97), 42, 14, 640, True, None),
    ("downscale_nonint", (97, 131), 42, 14, 640, False, None),
    ("upscale", (30, 30), 42, 14, 640, True, None),
    ("ratio16_33taps", (224, 224), 14, 14, 640, True, None),
    ("patch_s45_p14_drops_cols", (50, 50), 45, 14, 640, True, None),
    ("patch_kp_eq_3pp_p16", (40, 40), 32, 16, 768, True, None),
    ("mix_fixed_point_lam0", (97, 131), 42, 14, 640, False, 0.0),
    ("mix_fixed_point_lam0.3", (97, 131), 42, 14, 640, True, 0.3),
    ("mix_fixed_point_lam1", (30, 30), 42, 14, 640, False, 1.0),
]
INST = [(u8, dt) for u8 in (True, False) for dt in (F32, BF16, F16)]
INST_IDS = [f"{'u8' if u8 else 'f32src'}_{kr.DT_NAME[dt]}" for u8, dt in INST]


@pytest.mark.parametrize("u8,dtype", INST, ids=INST_IDS)
@pytest.mark.parametrize("geom", PRE_GEOM, ids=lambda gm: gm[0])
def test_preprocess_branches(lib, geom, u8, dtype):
    """All six preprocess_kernel instantiations at every resample branch and both layouts.  Patch-major pad columns have
    bound 0 (exactly zero); with S % P != 0 the pixels past the last whole patch are absent from the operand."""
    name, (Hs, Ws), S, Pp, Kp, patch, lam = geom
    B = 3
    src = kr.image_source(B, Hs, Ws, u8, seed=len(name) + Hs)
    mix = None if lam is None else torch.tensor([1, 1, 0], dtype=torch.int32)          # image 1 is a fixed point
    tdt = tdt_of(dtype)
    out = out_buffer(B, S, Pp, Kp, patch, tdt)
    src_d, mix_d = src.to(DEV), None if mix is None else mix.to(DEV)   # named: alive until the kernel has run
    ok(preprocess(lib, src_d, u8, out.ptr, dtype, B, Hs, Ws, S, Pp, Kp, patch, mix_d, 1.0 if lam is None else lam))
    what = f"preprocess {name} {'u8' if u8 else 'f32'}->{kr.DT_NAME[dtype]}"
    out.check(what)
    ref, bound = kr.preprocess_ref(src, u8, S, Pp, Kp, patch, 0.5, 0.5, mix, lam, tdt)
    got = out.got() if patch else out.got().view(B, 3, S, S)
    within(got, ref, bound, what)
    if patch and Kp > 3 * Pp * Pp:
        assert bool((out.got()[:, 3 * Pp * Pp:] == 0).all()), f"{what}: pad columns not exactly zero"


def test_preprocess_grid_stride(lib):
    """6 x 3 x 512 x 512 = 4 718 592 outputs, more than the 16384 x 256 threads of the capped grid: the grid-stride loop's
    second trip (a small source up-sampled, so the taps stay two per axis)."""
    B, Hs, S = 6, 64, 512
    assert B * 3 * S * S > 16384 * 256
    src = kr.image_source(B, Hs, Hs, True, seed=9)
    out = out_buffer(B, S, 14, 640, False, torch.bfloat16)
    src_d = src.to(DEV)
    ok(preprocess(lib, src_d, True, out.ptr, BF16, B, Hs, Hs, S, 14, 640, False))
    out.check("preprocess grid-stride")
    ref, bound = kr.preprocess_ref(src, True, S, 14, 640, False, 0.5, 0.5, None, 1.0, torch.bfloat16)
    within(out.got().view(B, 3, S, S), ref, bound, "preprocess grid-stride")


@pytest.mark.parametrize("entry", ["preprocess", "preprocess_aug"])
def test_preprocess_argument_errors_write_nothing(lib, entry):
    """A ratio just above 16 is SGL_ERR_UNSUPPORTED; std == 0, Kp < 3 P^2, S < P, a NULL pointer and a bad dtype code are
    refused too; each with the output's NaN body (and grey_mean's) untouched."""
    B = 2
    src = kr.image_source(B, 225, 225, True, seed=3).to(DEV)
    tab = aug_device_table(kr.aug_table()[:B])
    out = out_buffer(B, 14, 14, 640, True, torch.bfloat16)
    gm = flat(B, torch.float32)

    def call(src_=src, Hs=224, out_=out.ptr, dt=BF16, S=14, Pp=14, Kp=640, std=0.5, tab_=tab, gm_=gm.ptr):
        if entry == "preprocess":
            return lib.sgl_op_preprocess(P(src_), 1, B, Hs, Hs, out_, dt, S, Pp, Kp, 1, 0.5, std, None, 1.0, stream())
        return lib.sgl_op_preprocess_aug(P(src_), 1, B, Hs, Hs, out_, dt, S, Pp, Kp, 1, 0.5, std, P(tab_), gm_, stream())
    assert call(Hs=225) == UNSUPPORTED                   # 225 / 14 = 16.07
    assert call(std=0.0) == BAD_SHAPE
    assert call(Kp=587) == BAD_SHAPE
    assert call(S=13) == BAD_SHAPE
    assert call(src_=None) == NULL and call(out_=None) == NULL
    assert call(dt=2) == UNSUPPORTED and call(dt=4) == UNSUPPORTED
    if entry == "preprocess_aug":
        assert call(tab_=None) == NULL and call(gm_=None) == NULL
    torch.cuda.synchronize()
    untouched(out, entry)
    untouched(gm, entry + " grey_mean")


# =========================================================================================================
# sgl_op_preprocess_aug
# =========================================================================================================
def aug_device_table(tab):
    """sgl_aug_sample records (7 floats, 4 ints, 1 reserved int: 48 bytes) on the device."""
    fl = torch.tensor([[t[k] for k in kr.AUG_FIELDS[:-1]] for t in tab], dtype=torch.float32).view(torch.int32)
    it = torch.tensor([list(t["order"]) + [0] for t in tab], dtype=torch.int32)
    rec = torch.cat([fl, it], 1).contiguous()
    assert rec.shape[1] * 4 == 48
    return rec.to(DEV)


@pytest.mark.parametrize("case", kr.AUG_CASES, ids=lambda c: c[0])
def test_preprocess_aug_branches(lib, case):
    """All six preprocess_aug_kernel instantiations, both aug_mean_kernel variants and the three patch_pad_zero_kernel
    variants.  The table has one image per branch (kernel_ref.aug_table): no-op, flip only, rotation of either sign, the
    (1, 0) shortcut, order[0] < 0, contrast first / last / absent, each operator alone.  grey_mean is an output too:
    guarded, bounded, and exactly 0 where the chain has no contrast step."""
    name, u8, dtype, (Hs, Ws), S, Pp, Kp, patch = case
    src, tab = kr.aug_case_inputs(name)
    B = len(tab)
    tdt = tdt_of(dtype)
    out = out_buffer(B, S, Pp, Kp, patch, tdt)
    gm = flat(B, torch.float32)
    src_d, tab_d = src.to(DEV), aug_device_table(tab)                 # named: alive until the kernels have run
    ok(lib.sgl_op_preprocess_aug(P(src_d), int(u8), B, Hs, Ws, out.ptr, dtype, S, Pp, Kp, int(patch), 0.5, 0.5, P(tab_d),
                                 gm.ptr, stream()))
    what = f"preprocess_aug {name}"
    out.check(what)
    gm.check(what + " grey_mean")
    ref, bound, gref, gbound, mask = kr.aug_ref(src, u8, S, tab, 0.5, 0.5, tdt)
    assert mask.float().mean((1, 2)).max().item() <= kr.HUE_EXCUSED_CAP            # per image, not diluted over the case
    within(gm.got().view(B), gref, gbound, what + " grey_mean")
    keep = (~mask)[:, None].expand_as(ref)
    if patch:
        ref, bound = kr.patch_major(ref, bound, Pp, Kp)
        keep = kr.patch_major(keep.double(), keep.double(), Pp, Kp)[0] > 0
        keep[:, 3 * Pp * Pp:] = True                                                   # pad columns: never excused
        got = out.got().cpu()
        assert bool((got[:, 3 * Pp * Pp:] == 0).all()), f"{what}: pad columns not exactly zero"
    else:
        got = out.got().view(B, 3, S, S).cpu()
    within(got[keep], ref[keep], bound[keep], what)


# =========================================================================================================
# sgl_op_l2norm_tmean_fwd / _bwd
# =========================================================================================================
@pytest.mark.parametrize("B,T,D", kr.L2_SHAPES, ids=str)
def test_l2norm_tmean_shapes_and_extreme_norms(lib, B, T, D):
    """D = 1, D below / above one 256-thread trip, the model's 1152, and the header's largest D (16380: D * 4 + 16 bytes of
    LDS is exactly 64 KiB).  Frame 0 has norm 1e-18 (squares at the bottom of fp32's normal range: the bound's subnormal
    term), the last frame 1e18.  The backward reads the forward's own inv_norm."""
    f, g = kr.l2_inputs(B, T, D, seed=B * 10 + T)
    out, inv, df = Guarded(B, D, D, torch.float32), flat(B * T, torch.float32), Guarded(B * T, D, D, torch.float32)
    fd, gd = f.to(DEV), g.to(DEV)
    ok(lib.sgl_op_l2norm_tmean_fwd(P(fd), out.ptr, inv.ptr, B, T, D, stream()))
    what = f"l2norm_tmean B={B} T={T} D={D}"
    out.check(what + " out")
    inv.check(what + " inv_norm")
    (ro, bo), (ri, bi) = kr.l2norm_tmean_fwd_ref(f, B, T)
    within(out.got(), ro, bo, what + " out")
    within(inv.got().view(-1), ri, bi, what + " inv_norm")
    inv_dev = inv.got().reshape(-1).contiguous()
    ok(lib.sgl_op_l2norm_tmean_bwd(P(fd), P(inv_dev), P(gd), df.ptr, B, T, D, stream()))
    df.check(what + " df")
    rd, bd = kr.l2norm_tmean_bwd_ref(f, inv_dev.cpu(), g, B, T)
    within(df.got(), rd, bd, what.replace("l2norm_tmean", "l2norm_tmean_bwd") + " df")


def test_l2norm_tmean_refuses_d_above_the_limit(lib):
    D = kr.L2_MAX_D + 1
    f = torch.ones(1, D, device=DEV)
    out, inv = Guarded(1, D, D, torch.float32), flat(1, torch.float32)
    assert lib.sgl_op_l2norm_tmean_fwd(P(f), out.ptr, inv.ptr, 1, 1, D, stream()) == BAD_SHAPE
    torch.cuda.synchronize()
    untouched(out, "l2norm D over the limit")
    untouched(inv, "l2norm D over the limit, inv_norm")


# =========================================================================================================
# sgl_op_dwconv3x3
# =========================================================================================================
def dw_inputs(dtype, B, gh, gw, E, seed):
    g = gen(seed)
    tdt = tdt_of(dtype)
    x = randn(g, B, gh, gw, E).to(tdt)
    dy = randn(g, B, gh, gw, E).to(tdt)
    w9 = randn(g, 9, E)                               # nine distinct taps per channel
    bias = randn(g, E)
    return x, dy, w9, bias


@pytest.mark.parametrize("flip,with_bias", [(0, True), (0, False), (1, False), (1, True)],
                         ids=["fwd_bias", "fwd_nobias", "flip_nobias", "flip_bias"])
@pytest.mark.parametrize("grid", [(1, 1), (1, 7), (7, 1), (5, 7)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("E_of", ["one_vector", 64, "256_vectors"], ids=str)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: kr.DT_NAME[d])
def test_dwconv3x3_branches(lib, dtype, E_of, grid, flip, with_bias):
    """One channel vector per pixel (E = nv), 64 channels, and 256 vectors per pixel (E = 1024 for fp32, where 256 % 256
    == 0 is the last admitted divisor; bf16's 1024 is 128 vectors) on degenerate and odd grids: every border pixel has its
    own tap count in the bound."""
    nv = kr.NV[dtype]
    E = nv if E_of == "one_vector" else (1024 if E_of == "256_vectors" else 64)
    gh, gw = grid
    B = 2
    x, _, w9, bias = dw_inputs(dtype, B, gh, gw, E, seed=E + gh * 8 + gw + flip)
    tdt = tdt_of(dtype)
    y = Guarded(B * gh * gw, E, E, tdt)
    ok(lib.sgl_op_dwconv3x3(P(x), dtype, P(w9), P(bias) if with_bias else None, y.ptr, B, gh, gw, E, flip, stream()))
    what = f"dwconv {kr.DT_NAME[dtype]} E={E} {gh}x{gw} flip={flip} bias={with_bias}"
    y.check(what)
    ref, bound = kr.dwconv_ref(x, w9, bias if with_bias else None, flip, tdt)
    within(y.got().view(B, gh, gw, E), ref, bound, what)


def test_dwconv3x3_grid_stride(lib):
    """2049 x 2048 pixels of one fp32 channel vector each: 4 196 352 work items, above the 16384 x 256 cap."""
    B, gh, gw, E = 1, 2049, 2048, 4
    assert B * gh * gw * (E // 4) > 16384 * 256
    x, _, w9, bias = dw_inputs(F32, B, gh, gw, E, seed=77)
    y = Guarded(B * gh * gw * E // 4096, 4096, 4096, torch.float32)
    ok(lib.sgl_op_dwconv3x3(P(x), F32, P(w9), P(bias), y.ptr, B, gh, gw, E, 1, stream()))
    y.check("dwconv grid-stride")
    ref, bound = kr.dwconv_ref(x, w9, bias, 1, torch.float32)
    within(y.got().view(B, gh, gw, E), ref, bound, "dwconv grid-stride")


def test_dwconv3x3_refusals_write_nothing(lib):
    """bf16 E = 24 fails 256 % (E / 8) == 0; a pointer 4 bytes off 16-byte alignment is refused as well (x, y, w9, bias):
    no launch, the output untouched."""
    x, _, w9, bias = dw_inputs(BF16, 1, 3, 3, 24, seed=1)
    y = Guarded(9, 24, 24, torch.bfloat16)
    assert lib.sgl_op_dwconv3x3(P(x), BF16, P(w9), P(bias), y.ptr, 1, 3, 3, 24, 0, stream()) == BAD_SHAPE
    x, _, w9, bias = dw_inputs(F32, 1, 3, 3, 64, seed=2)
    y2 = Guarded(9, 64, 64, torch.float32)
    big = torch.zeros(9 * 64 + 16, device=DEV)
    for a in ((big[1:].data_ptr(), P(w9), P(bias), y2.ptr), (P(x), big[1:].data_ptr(), P(bias), y2.ptr),
              (P(x), P(w9), big[1:].data_ptr(), y2.ptr), (P(x), P(w9), P(bias), y2.ptr + 4)):
        assert lib.sgl_op_dwconv3x3(a[0], F32, a[1], a[2], a[3], 1, 3, 3, 64, 0, stream()) == BAD_SHAPE
    torch.cuda.synchronize()
    untouched(y, "dwconv E=24")
    untouched(y2, "dwconv misaligned")


def test_dwconv_wrapper_copies_a_misaligned_operand(pkg, lib):
    """head_ops._DepthwiseConv3x3Fn on an input, a bias and an upstream gradient that are contiguous views 4 bytes into their
    buffers (`.contiguous()` leaves such a view where it is): correct values, forward and backward."""
    H = pkg.head_ops
    B, gh, gw, E = 2, 5, 7, 64
    n = B * gh * gw * E
    g = gen(5)
    xb, db, bb = randn(g, n + 4), randn(g, n + 4), randn(g, E + 4)
    x = xb[1:n + 1].view(B, gh, gw, E).requires_grad_(True)
    dy = db[1:n + 1].view(B, gh, gw, E)
    bias = bb[1:E + 1].requires_grad_(True)
    weight = randn(g, E, 1, 3, 3).requires_grad_(True)
    assert x.data_ptr() % 16 and dy.data_ptr() % 16 and bias.data_ptr() % 16 and x.is_contiguous()
    y = H._DepthwiseConv3x3Fn.apply(x, weight, bias)
    dx, dw, dbias = torch.autograd.grad(y, (x, weight, bias), dy)
    w9 = weight.detach().reshape(E, 9).t().contiguous()
    ref, bound = kr.dwconv_ref(x.detach(), w9, bias.detach(), 0, torch.float32)
    within(y.detach(), ref, bound, "wrapper forward")
    ref, bound = kr.dwconv_ref(dy, w9, None, 1, torch.float32)
    within(dx, ref, bound, "wrapper dx")
    ref, bound = kr.dwconv_wgrad_ref(x.detach(), dy)
    within(torch.cat([dw.reshape(E, 9).t(), dbias[None]]), ref, bound, "wrapper dw, dbias")


# =========================================================================================================
# sgl_op_dwconv3x3_wgrad
# =========================================================================================================
WGRAD_CASES = [
    ("npix_lt_512", 2, 3, 5, 64),                     # 30 pixels: 30 blocks of one pixel
    ("short_last_block_straddles_images", 5, 5, 41, 64),   # 1025 pixels: 342 blocks of 3, the last holds 2; 205 per image
    ("one_vector", 3, 7, 9, None),                    # E = nv: 256 pixel lanes per block
]


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: kr.DT_NAME[d])
def test_dwconv3x3_wgrad_branches(lib, dtype, case, accumulate):
    """accumulate = 0 over a NaN prior (must vanish), accumulate = 1 over a finite prior (kept); one byte of scratch short
    is SGL_ERR_WORKSPACE with dw10 untouched."""
    name, B, gh, gw, E = case
    E = E or kr.NV[dtype]
    x, dy, _, _ = dw_inputs(dtype, B, gh, gw, E, seed=B + gh + gw)
    npix = B * gh * gw
    nblk = min(npix, 512)
    ppb = -(-npix // nblk)
    nblk = -(-npix // ppb)
    if "short" in name:
        assert npix % ppb and (gh * gw) % ppb
    need = nblk * 10 * E * 4
    assert need <= lib.sgl_op_dwconv3x3_wgrad_scratch_bytes(B, gh, gw, E)
    scratch = torch.empty(need // 4, device=DEV)
    prior = randn(gen(3), 10, E) if accumulate else None
    dw = Guarded(10, E, E, torch.float32, prior=prior)
    blank = Guarded(10, E, E, torch.float32)
    assert lib.sgl_op_dwconv3x3_wgrad(P(x), P(dy), dtype, blank.ptr, accumulate, P(scratch), need - 1, B, gh, gw, E,
                                      stream()) == WORKSPACE
    ok(lib.sgl_op_dwconv3x3_wgrad(P(x), P(dy), dtype, dw.ptr, accumulate, P(scratch), need, B, gh, gw, E, stream()))
    what = f"wgrad {kr.DT_NAME[dtype]} {name} acc={accumulate}"
    dw.check(what)
    untouched(blank, what + " (scratch one byte short)")
    ref, bound = kr.dwconv_wgrad_ref(x, dy, prior)
    within(dw.got(), ref, bound, what)


def wgrad_order_child(order):
    """Body of the child process of test_dwconv3x3_wgrad_first_call_of_either_type: the two kernels in the given order in a
    process that has launched neither (the 80 KiB LDS attribute of the bf16 kernel is set lazily, on whichever call
    comes first)."""
    import __graft_entry__ as entry
    hl = entry.load_package().lib.load()
    for dtype in ((F32, BF16) if order == "f32_first" else (BF16, F32)):
        B, gh, gw, E = 2, 5, 7, 64
        x, dy, _, _ = dw_inputs(dtype, B, gh, gw, E, seed=11)
        need = hl.sgl_op_dwconv3x3_wgrad_scratch_bytes(B, gh, gw, E)
        scratch = torch.empty(need // 4, device=DEV)
        dw = Guarded(10, E, E, torch.float32)
        ok(hl.sgl_op_dwconv3x3_wgrad(P(x), P(dy), dtype, dw.ptr, 0, P(scratch), need, B, gh, gw, E, stream()))
        dw.check(order)
        ref, bound = kr.dwconv_wgrad_ref(x, dy)
        within(dw.got(), ref, bound, f"wgrad {order} {kr.DT_NAME[dtype]}")
    print("WGRAD_ORDER_OK")


@pytest.mark.parametrize("order", ["f32_first", "bf16_first"])
def test_dwconv3x3_wgrad_first_call_of_either_type(order):
    """What this test is about needs a process of its own: the first weight-gradient call of a process being the fp32
    kernel, and being the bf16 one."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; "
            f"import test_kernel_edges_aux_gpu as t; t.wgrad_order_child({order!r})")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WGRAD_ORDER_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# =========================================================================================================
# sgl_op_gate_mul / _bwd
# =========================================================================================================
def gate_inputs(dtype, n, seed):
    g = gen(seed)
    tdt = tdt_of(dtype)
    gate = randn(g, n) * 4
    k = min(n, len(kr.GATE_SWEEP))
    gate[:k] = torch.tensor(kr.GATE_SWEEP[:k], device=DEV)
    x, dy = randn(g, n), randn(g, n)
    if n >= 2 * len(kr.GATE_SWEEP):                   # the saturating gates again, against large x and dy
        gate[k:2 * k] = gate[:k]
        x[k:2 * k] *= 1e3
        dy[k:2 * k] *= 1e3
    return gate.to(tdt), x.to(tdt), dy.to(tdt)


GATE_N = [("one_vector", lambda nv: nv), ("three_blocks_and_a_vector", lambda nv: 256 * nv * 3 + nv),
          ("grid_stride", lambda nv: 8192 * 256 * nv + 4096)]


@pytest.mark.parametrize("size", GATE_N, ids=lambda s: s[0])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: kr.DT_NAME[d])
def test_gate_mul_forward_sizes_and_gate_sweep(lib, dtype, size):
    """One vector; three blocks and one vector; more vectors than the 8192 x 256 threads of the capped grid.  The gates
    sweep 0, +-1e-3, +-20, +-88, +-104, +-200 (bf16: at their rounded values): exp2 saturates to inf and underflows to 0,
    and the bound grows with |g| as the rounded exponent's error does."""
    n = size[1](kr.NV[dtype])
    gate, x, _ = gate_inputs(dtype, n, seed=n % 1000)
    tdt = tdt_of(dtype)
    y = flat(n, tdt)
    ok(lib.sgl_op_gate_mul(P(gate), P(x), y.ptr, n, dtype, stream()))
    what = f"gate_mul {kr.DT_NAME[dtype]} {size[0]}"
    y.check(what)
    ref, bound = kr.gate_mul_ref(gate, x, tdt)
    within(y.got().reshape(-1), ref, bound, what)


# every destination combination at the two small sizes; the grid-stride trip once, with both destinations
GATE_BWD = [(s, nl) for s in GATE_N[:2] for nl in ("none", "dg", "dx", "both")] + [(GATE_N[2], "none")]


@pytest.mark.parametrize("size,null", GATE_BWD, ids=lambda v: v if isinstance(v, str) else v[0])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: kr.DT_NAME[d])
def test_gate_mul_backward_null_destinations(lib, dtype, size, null):
    """dg NULL, dx NULL, both: the buffer that is not passed keeps its guards AND its NaN body."""
    n = size[1](kr.NV[dtype])
    gate, x, dy = gate_inputs(dtype, n, seed=n % 1000 + 1)
    tdt = tdt_of(dtype)
    dg, dx = flat(n, tdt), flat(n, tdt)
    pg = None if null in ("dg", "both") else dg.ptr
    px = None if null in ("dx", "both") else dx.ptr
    ok(lib.sgl_op_gate_mul_bwd(P(dy), P(gate), P(x), pg, px, n, dtype, stream()))
    what = f"gate_mul_bwd {kr.DT_NAME[dtype]} {size[0]} null={null}"
    (rdg, bdg), (rdx, bdx) = kr.gate_mul_bwd_ref(dy, gate, x, tdt)
    for buf, p_, ref, bound, nm in ((dg, pg, rdg, bdg, "dg"), (dx, px, rdx, bdx, "dx")):
        if p_ is None:
            untouched(buf, f"{what}: {nm}")
        else:
            buf.check(f"{what}: {nm}")
            within(buf.got().reshape(-1), ref, bound, f"{what}: {nm}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: kr.DT_NAME[d])
def test_gate_mul_refusals_write_nothing(lib, dtype):
    nv = kr.NV[dtype]
    n = 4 * nv
    gate, x, dy = gate_inputs(dtype, n + nv, seed=1)
    tdt = tdt_of(dtype)
    y, dg, dx = flat(n, tdt), flat(n, tdt), flat(n, tdt)
    off = gate[1:].data_ptr()                         # 4 (fp32) or 2 (bf16) bytes off
    assert lib.sgl_op_gate_mul(P(gate), P(x), y.ptr, n + 1, dtype, stream()) == BAD_SHAPE
    assert lib.sgl_op_gate_mul(off, P(x), y.ptr, n, dtype, stream()) == BAD_SHAPE
    assert lib.sgl_op_gate_mul(P(gate), P(x), y.ptr + 4, n, dtype, stream()) == BAD_SHAPE
    assert lib.sgl_op_gate_mul_bwd(P(dy), P(gate), P(x), dg.ptr, dx.ptr, n - 1, dtype, stream()) == BAD_SHAPE
    assert lib.sgl_op_gate_mul_bwd(P(dy), off, P(x), dg.ptr, dx.ptr, n, dtype, stream()) == BAD_SHAPE
    assert lib.sgl_op_gate_mul_bwd(P(dy), P(gate), P(x), dg.ptr + 8, dx.ptr, n, dtype, stream()) == BAD_SHAPE
    torch.cuda.synchronize()
    for b in (y, dg, dx):
        untouched(b, "gate_mul refusal")


@pytest.mark.parametrize("which", ["gate", "x", "both"])
def test_gate_mul_wrapper_falls_back_on_an_offset_view(pkg, lib, which):
    """head_ops.gate_mul on 4096-element views that start 4 bytes into an fp32 buffer: sgl_op_gate_mul refuses such a pointer
    and `.contiguous()` does not move a contiguous view, so the wrapper computes sigmoid(g) * x itself, forward and
    backward (bit-identical to torch's composition: it IS that composition)."""
    H = pkg.head_ops
    n = 4096
    g = gen(21)
    gb, xb = randn(g, n + 8).requires_grad_(True), randn(g, n + 8).requires_grad_(True)
    og, ox = (1 if which in ("gate", "both") else 0), (1 if which in ("x", "both") else 0)
    gate, x = gb[og:og + n], xb[ox:ox + n]
    assert (gate.data_ptr() % 16 != 0) == bool(og) and (x.data_ptr() % 16 != 0) == bool(ox)
    dy = randn(g, n)
    y = H.gate_mul(gate, x)
    dgb, dxb = torch.autograd.grad(y, (gb, xb), dy)
    gr, xr = gb.detach().clone().requires_grad_(True), xb.detach().clone().requires_grad_(True)
    yr = torch.sigmoid(gr[og:og + n]) * xr[ox:ox + n]
    rg, rx = torch.autograd.grad(yr, (gr, xr), dy)
    assert torch.equal(y, yr) and torch.equal(dgb, rg) and torch.equal(dxb, rx)


def test_gate_mul_wrapper_accepts_an_offset_upstream_gradient(pkg, lib):
    """Aligned operands take the kernel; an upstream gradient that is an offset view is copied, not refused."""
    H = pkg.head_ops
    n = 4096
    g = gen(22)
    gate, x = (randn(g, n) * 3).requires_grad_(True), randn(g, n).requires_grad_(True)
    dy = randn(g, n + 4)[1:n + 1]
    assert dy.data_ptr() % 16 and dy.is_contiguous()
    y = H.gate_mul(gate, x)
    dgate, dx = torch.autograd.grad(y, (gate, x), dy)
    ref, bound = kr.gate_mul_ref(gate.detach(), x.detach(), torch.float32)
    within(y.detach(), ref, bound, "wrapper y")
    (rdg, bdg), (rdx, bdx) = kr.gate_mul_bwd_ref(dy, gate.detach(), x.detach(), torch.float32)
    within(dgate, rdg, bdg, "wrapper dg")
    within(dx, rdx, bdx, "wrapper dx")


# =========================================================================================================
# sgl_op_seg_loss_fwd / _bwd
# =========================================================================================================
@pytest.mark.parametrize("g,S", kr.SEG_CASES, ids=str)
def test_seg_loss_branches(lib, g, S):
    """(1, 8) one logit; (4, 56) integer ratio; (3, 42) non-integer ratio with a last chunk of 2 rows; (27, 320) S above one
    256-column trip; (16, 257) a one-column tail; (14, 14) scale 1; (27, 14) down-sampling.  Logits reach +-30 in part of
    the map; image 0 has an all-zero mask, image 1 an all-one mask, image 2 zero coefficients (dlogits_lr exactly 0), and
    image 3 a random mask under a band of ones with non-zero coefficients: the backward's mask read and its dice term at
    mixed t are held to the bound there.
    Every partial and every dlogits_lr element is held to its bound; two launches give identical bits."""
    B, eps = kr.SEG_B, 1e-6
    lr, tgt, coef = kr.seg_inputs(B, g, S, seed=g * 1000 + S)
    chunks = lib.sgl_op_seg_loss_chunks(S)
    assert chunks == (S + 7) // 8
    lrd, td, cd = lr.to(DEV), tgt.to(DEV), coef.to(DEV)
    what = f"seg_loss g={g} S={S}"
    parts = []
    for _ in range(2):
        part = Guarded(B * chunks, 4, 4, torch.float32)
        ok(lib.sgl_op_seg_loss_fwd(P(lrd), P(td), part.ptr, B, g, S, stream()))
        part.check(what + " partial")
        parts.append(part.got().clone())
    assert torch.equal(parts[0], parts[1]), f"{what}: forward not bitwise reproducible"
    ref, bound = kr.seg_loss_fwd_ref(lr, tgt)
    within(parts[0].view(B, chunks, 4), ref, bound, what + " partial")
    sums = parts[0].view(B, chunks, 4).double().sum(1).float().contiguous()            # the caller's fold
    outs = []
    for _ in range(2):
        dl = Guarded(B * g, g, g, torch.float32)
        ok(lib.sgl_op_seg_loss_bwd(P(lrd), P(td), P(sums), P(cd), dl.ptr, B, g, S, eps, stream()))
        dl.check(what + " dlogits_lr")
        outs.append(dl.got().clone())
    assert torch.equal(outs[0], outs[1]), f"{what}: backward not bitwise reproducible"
    dref, dbound = kr.seg_loss_bwd_ref(lr, tgt, sums.cpu(), coef, eps)
    within(outs[0].view(B, g, g), dref, dbound, what.replace("seg_loss", "seg_loss_bwd") + " dlogits_lr")
    assert bool((outs[0].view(B, g, g)[2] == 0).all()), f"{what}: zero coefficients must give exact zeros"


def test_seg_loss_shape_limits_write_nothing(lib):
    lr, tgt, coef = kr.seg_inputs(1, 3, 42, seed=1)
    lrd, td, cd = lr.to(DEV), tgt.to(DEV), coef.to(DEV)
    part, dl = Guarded(6, 4, 4, torch.float32), Guarded(3, 3, 3, torch.float32)
    sums = torch.ones(4, device=DEV)
    for b, g, s in ((0, 3, 42), (1, 0, 42), (1, 3, 0), (1, 4097, 42), (1, 3, 16385)):
        assert lib.sgl_op_seg_loss_fwd(P(lrd), P(td), part.ptr, b, g, s, stream()) == BAD_SHAPE
    for b, g, s in ((0, 3, 42), (1, 0, 42), (1, 3, 0), (1, 4097, 42), (1, 3, 8193)):
        assert lib.sgl_op_seg_loss_bwd(P(lrd), P(td), P(sums), P(cd), dl.ptr, b, g, s, 1e-6, stream()) == BAD_SHAPE
    torch.cuda.synchronize()
    untouched(part, "seg_loss_fwd limits")
    untouched(dl, "seg_loss_bwd limits")


# =========================================================================================================
# sgl_op_adamw
# =========================================================================================================
SENT = 0x5A5A5A5A
# (elements, which of p, g, m, v start 4 bytes off 16-byte alignment, has a gradient)
ADAMW_ENTRIES = [(4096, "", True), (4097, "p", True), (3, "g", True), (12289, "pgmv", True), (1, "", True),
                 (12289, "", True), (4097, "", False), (3, "pgmv", True), (1, "pgmv", True)]


class Arena:
    """One fp32 buffer of sentinel bit patterns from which tensors are cut with a chosen alignment and 32-float gaps."""

    def __init__(self, total):
        self.buf = torch.empty(total, device=DEV, dtype=torch.float32)
        self.buf.view(torch.int32).fill_(SENT)
        self.live = torch.zeros(total, dtype=torch.bool, device=DEV)
        self.at = 32

    def take(self, n, off):
        start = (self.at + 3) // 4 * 4 + (1 if off else 0)
        self.at = start + n + 32
        assert self.at <= self.buf.numel()
        self.live[start:start + n] = True
        t = self.buf[start:start + n]
        assert (t.data_ptr() % 16 == 4) == bool(off) and (off or t.data_ptr() % 16 == 0)
        return t

    def guards_intact(self):
        return bool((self.buf.view(torch.int32)[~self.live] == SENT).all())


def adamw_setup(pkg, seed):
    """The table on a fresh arena: host copies of the values, the device table, the plan."""
    L = pkg.lib
    g = torch.Generator().manual_seed(seed)
    arena = Arena(sum(n for n, _, _ in ADAMW_ENTRIES) * 4 + 64 * 4 * len(ADAMW_ENTRIES) + 64)
    table = (L.SglAdamwTensor * len(ADAMW_ENTRIES))()
    host, views = [], []
    for i, (n, off, has_g) in enumerate(ADAMW_ENTRIES):
        vals = dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g) * 0.01,
                    m=torch.randn(n, generator=g) * 0.01, v=torch.rand(n, generator=g) * 1e-4)
        if n >= 3:
            vals["g"][0] = 0.0
            vals["v"][1] = 0.0
        lr, wd = 1e-3 * (1 + i), 0.01 * i
        view = {k: arena.take(n, k in off) for k in "pgmv"}
        for k in "pgmv":
            view[k].copy_(vals[k])
        table[i].p, table[i].m, table[i].v = view["p"].data_ptr(), view["m"].data_ptr(), view["v"].data_ptr()
        table[i].g = view["g"].data_ptr() if has_g else None
        table[i].n, table[i].lr, table[i].weight_decay = n, lr, wd
        host.append((vals, lr, wd, has_g))
        views.append(view)
    numel = (C.c_uint64 * len(ADAMW_ENTRIES))(*[n for n, _, _ in ADAMW_ENTRIES])
    lib_ = L.load()
    nb = lib_.sgl_adamw_plan(numel, len(ADAMW_ENTRIES), None, 0)
    bm = (C.c_int32 * (2 * nb))()
    assert lib_.sgl_adamw_plan(numel, len(ADAMW_ENTRIES), bm, nb) == nb
    dev_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    dev_map = torch.tensor(list(bm), dtype=torch.int32, device=DEV)
    return arena, views, host, dev_table, dev_map, nb


@pytest.mark.parametrize("clip", [None, 0.37], ids=["noclip", "clip0.37"])
@pytest.mark.parametrize("step", [1, 1000])
def test_adamw_table_elementwise_and_bitwise_equal_to_ex(pkg, lib, step, clip):
    """adamw_kernel over a table that mixes aligned tensors with ones 4 bytes off (only p, only g, all four), sizes 1, 3,
    4096, 4097, 12289 and an entry without a gradient (left bit-identical): every p, exp_avg, exp_avg_sq element against
    the float64 step, the gaps between the tensors untouched, and the whole arena BIT-IDENTICAL to sgl_op_adamw_ex on the
    same table with an all-NULL aux and group = -1 (adamw_one is shared and compiled contraction-off)."""
    L = pkg.lib
    b1, b2, eps = 0.9, 0.999, 1e-8
    nc = None if clip is None else torch.tensor([3.3, clip], device=DEV)
    arena, views, host, table, bmap, nb = adamw_setup(pkg, seed=step)
    before = arena.buf.clone()
    ok(lib.sgl_op_adamw(P(table), P(bmap), nb, b1, b2, eps, step, P(nc), stream()))
    assert arena.guards_intact(), "adamw wrote between the tensors"
    for i, ((vals, lr, wd, has_g), view) in enumerate(zip(host, views)):
        what = f"adamw entry {i} n={ADAMW_ENTRIES[i][0]} off={ADAMW_ENTRIES[i][1]!r} step={step}"
        assert torch.equal(view["g"].cpu(), vals["g"]), what + ": the gradient was modified"
        if not has_g:
            for k in "pmv":
                assert torch.equal(view[k].cpu(), vals[k]), what + f": {k} changed without a gradient"
            continue
        refs = kr.adamw_ref(vals["p"], vals["g"], vals["m"], vals["v"], lr, wd, b1, b2, eps, step,
                            None if clip is None else nc[1].item())
        for k, (ref, bound) in zip("pmv", refs):
            within(view[k], ref, bound, f"{what} {k}")
    arena2, _, _, table2, bmap2, nb2 = adamw_setup(pkg, seed=step)
    assert torch.equal(arena2.buf.view(torch.int32), before.view(torch.int32))
    aux = (L.SglAdamwAux * len(ADAMW_ENTRIES))()
    for a in aux:
        a.group = -1
    dev_aux = torch.frombuffer(bytearray(bytes(aux)), dtype=torch.uint8).to(DEV)
    ok(lib.sgl_op_adamw_ex(P(table2), P(dev_aux), P(bmap2), nb2, b1, b2, eps, step, P(nc), None, 0, 0.0, stream()))
    assert torch.equal(arena.buf.view(torch.int32), arena2.buf.view(torch.int32)), "adamw and adamw_ex differ in bits"


def test_adamw_step_zero_is_refused(pkg, lib):
    arena, _, _, table, bmap, nb = adamw_setup(pkg, seed=5)
    before = arena.buf.clone()
    assert lib.sgl_op_adamw(P(table), P(bmap), nb, 0.9, 0.999, 1e-8, 0, None, stream()) == BAD_SHAPE
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), arena.buf.view(torch.int32))
