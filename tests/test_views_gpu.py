"""GPU: sgl_op_preprocess_views, the app's test-time views (crop -> quarter turn -> mirror -> resize -> normalise) of B
same-size sources in one pass, through the C ABI and up to `model(patches=views_to_patch_operand(...))`.

The discipline of tests/test_preprocess_bwd_gpu.py: every element is held to its own derived bound against the float64
reference of tests/views_ref.py (pinned to PIL on the CPU in tests/test_views_host.py), outputs sit between sentinel guard
rows with a NaN body, each case is named after the branch it is there for and prints its worst err/bound as a RATIO line
before it asserts, and refusals write nothing.  S = 42, P = 14, Kp = 640 unless a case names another.
"""
import pytest
import torch

import kernel_ref as kr
import views_ref as vr
from kernel_ref import BF16, F16, F32
from test_input_grad_gpu import build
from test_kernel_edges_aux_gpu import BAD_SHAPE, NULL, UNSUPPORTED, out_buffer, preprocess, untouched, within
from test_kernel_edges_gpu import DEV, P, lib, ok, stream, tdt_of  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu
CHUNK = 64                                   # records per launch (kViewChunk of csrc/preprocess.hip)
INST = [(u8, dt) for u8 in (True, False) for dt in (F32, BF16, F16)]
INST_IDS = [f"{'u8' if u8 else 'f32src'}_{kr.DT_NAME[dt]}" for u8, dt in INST]


def table(pkg, views):
    """ctypes sgl_view[V] of plain (src, box, turns, keep_canvas, flip) tuples, unchecked (refusals need bad ones)."""
    return (pkg.lib.SglView * len(views))(*(pkg.lib.SglView(b, *box, t, int(k), int(f)) for b, box, t, k, f in views))


def run_views(pkg, lib, src_d, u8, views, out_ptr, dtype, S, Pp=14, Kp=640, patch=True, mean=0.5, std=0.5):
    B = src_d.shape[0]
    Hs, Ws = (src_d.shape[1], src_d.shape[2]) if u8 else (src_d.shape[2], src_d.shape[3])
    tab = table(pkg, views)
    nbytes = lib.sgl_op_preprocess_views_scratch_bytes(len(views), S)
    scratch = torch.empty(nbytes, device=DEV, dtype=torch.uint8) if nbytes else None
    st = lib.sgl_op_preprocess_views(P(src_d), int(u8), B, Hs, Ws, tab, len(views), out_ptr, dtype, S, Pp, Kp, int(patch),
                                     mean, std, P(scratch), nbytes, stream())
    torch.cuda.synchronize()                             # scratch stays alive until the kernels have run
    return st


def check_views(pkg, lib, what, src, u8, views, dtype, S, Pp=14, Kp=640, patch=True, mean=0.5, std=0.5):
    """One call on a guarded output, every element against its bound; returns the output (V rows of the layout)."""
    V, tdt = len(views), tdt_of(dtype)
    out = out_buffer(V, S, Pp, Kp, patch, tdt)
    src_d = src.to(DEV)
    ok(run_views(pkg, lib, src_d, u8, views, out.ptr, dtype, S, Pp, Kp, patch, mean, std))
    out.check(what)
    ref, bound = vr.views_ref(src, u8, views, S, Pp, Kp, patch, mean, std, tdt)
    got = out.got() if patch else out.got().view(V, 3, S, S)
    within(got, ref, bound, what)
    if patch and Kp > 3 * Pp * Pp:
        assert bool((out.got()[:, 3 * Pp * Pp:] == 0).all()), f"{what}: pad columns not exactly zero"
    return got


def plain(b, box):
    return (b, box, 0, False, False)


# ---- bit for bit against sgl_op_preprocess -----------------------------------------------------------------------
@pytest.mark.parametrize("u8,dtype", INST, ids=INST_IDS)
@pytest.mark.parametrize("S,patch", [(45, False), (42, True)], ids=["s45_nchw", "s42_patch"])
def test_full_frame_and_plain_crops_equal_preprocess_bitwise(pkg, lib, S, patch, u8, dtype):
    """The full frame equals sgl_op_preprocess on the same source, a plain crop equals it on the contiguous cropped copy:
    the same filter code, so the same bits.  Boxes: the frame; odd offsets; 42 wide (one axis the identity at S = 42);
    42 x 42 (the copy shortcut at S = 42); a box up-scaled on both axes."""
    B, Hs, Ws = 2, 50, 61
    src = kr.image_source(B, Hs, Ws, u8, seed=41)
    src_d = src.to(DEV)
    tdt = tdt_of(dtype)
    boxes = [(0, 0, Ws, Hs), (3, 5, 40, 47), (7, 1, 49, 50), (10, 4, 52, 46), (33, 17, 44, 30)]
    views = [plain(b, box) for b in range(B) for box in boxes]
    what = f"views bitwise {'u8' if u8 else 'f32'}->{kr.DT_NAME[dtype]} S{S} {'patch' if patch else 'nchw'}"
    got = check_views(pkg, lib, what, src, u8, views, dtype, S, patch=patch)
    rows = got.shape[0] // len(views)

    def expect(source_d, Bn, h, w):
        want = out_buffer(Bn, S, 14, 640, patch, tdt)
        ok(preprocess(lib, source_d, u8, want.ptr, dtype, Bn, h, w, S, 14, 640, patch))
        torch.cuda.synchronize()
        want.check(what)
        return want.got() if patch else want.got().view(Bn, 3, S, S)
    full = expect(src_d, B, Hs, Ws)
    for n, (b, (x0, y0, x1, y1), *_) in enumerate(views):
        mine = got[n * rows:(n + 1) * rows]
        if (x0, y0, x1, y1) == (0, 0, Ws, Hs):
            assert torch.equal(mine, full[b * rows:(b + 1) * rows]), f"{what}: full frame of image {b}"
        cut = (src_d[b:b + 1, y0:y1, x0:x1] if u8 else src_d[b:b + 1, :, y0:y1, x0:x1]).contiguous()
        assert torch.equal(mine, expect(cut, 1, y1 - y0, x1 - x0)), f"{what}: crop {(x0, y0, x1, y1)} of image {b}"


# ---- the branches ------------------------------------------------------------------------------------------------
def test_nine_crops_of_97x64(pkg, lib):
    views, _ = pkg.preprocess.multicrop_views(64, 97)
    src = kr.image_source(1, 64, 97, True, seed=42)
    check_views(pkg, lib, "views nine_crops_97x64 u8->bf16", src, True, [vr.as_tuple(v) for v in views], BF16, 42)


SCALES = [
    ("upscale_8x8_box", (13, 21, 21, 29), 42, 14),
    ("ratio16_33taps", (5, 9, 229, 233), 14, 14),
    ("one_axis_identity_w42", (101, 3, 143, 100), 42, 14),
    ("odd_offsets_nonint", (7, 11, 104, 142), 42, 14),
    ("copy_shortcut_42x42", (31, 57, 73, 99), 42, 14),
]


@pytest.mark.parametrize("u8,dtype", [(True, BF16), (False, F32), (True, F16)], ids=["u8_bf16", "f32src_f32", "u8_f16"])
@pytest.mark.parametrize("case", SCALES, ids=lambda c: c[0])
def test_scale_branches(pkg, lib, case, u8, dtype):
    name, box, S, Pp = case
    src = kr.image_source(2, 240, 235, u8, seed=len(name))
    views = [plain(1, box), plain(0, box)]
    for patch in (True, False):
        check_views(pkg, lib, f"views {name} {'u8' if u8 else 'f32'}->{kr.DT_NAME[dtype]} patch{int(patch)}", src, u8,
                    views, dtype, S, Pp, 640, patch)


# box (x0, y0, x1, y1): 51 x 34 (w - h odd), 50 x 34 (even), 37 x 37 (zero), 34 x 51 (odd, portrait)
ORIENT_BOXES = {"w-h_odd": (3, 5, 54, 39), "w-h_even": (4, 5, 54, 39), "square": (9, 2, 46, 39), "portrait_odd": (7, 1, 41, 52)}
ORIENT = [(f"{bn}_t{t}_{'canvas' if k else 'exact'}{'_flip' if f else ''}", box, t, k, f)
          for bn, box in ORIENT_BOXES.items() for t, k, f in
          [(1, False, False), (2, False, False), (3, False, False), (1, True, False), (2, True, False), (3, True, False),
           (0, False, True), (1, False, True), (1, True, True), (3, True, True)]]


@pytest.mark.parametrize("u8,dtype,patch", [(True, BF16, True), (False, F32, False), (True, F32, True)],
                         ids=["u8_bf16_patch", "f32src_f32_nchw", "u8_f32_patch"])
def test_orientation(pkg, lib, u8, dtype, patch):
    """Turns 1, 2, 3 exact and on the kept canvas for w - h odd, even and zero, flip alone and after a turn: forty views
    in one call, each element against the reference's oriented image (pinned to PIL in tests/test_views_host.py)."""
    src = kr.image_source(1, 56, 60, u8, seed=43)
    views = [(0, box, t, k, f) for _, box, t, k, f in ORIENT]
    check_views(pkg, lib, f"views orientation {'u8' if u8 else 'f32'}->{kr.DT_NAME[dtype]} patch{int(patch)}", src, u8,
                views, dtype, 42, patch=patch)


def test_kept_canvas_fill_is_exactly_minus_mean_over_std(pkg, lib):
    """A 48 x 6 strip turned on its canvas keeps a 6-wide band; output columns whose taps all lie in the fill are
    (0 - mean) / std exactly, in every channel."""
    src = kr.image_source(1, 20, 60, True, seed=44)
    views = [(0, (5, 7, 53, 13), 1, True, False), (0, (5, 7, 53, 13), 3, True, True)]
    got = check_views(pkg, lib, "views canvas_fill u8->f32", src, True, views, F32, 42, patch=False, mean=0.25, std=0.5)
    assert bool((got[:, :, :, :14] == -0.5).all()) and bool((got[:, :, :, 28:] == -0.5).all())
    assert bool((got[:, :, :, 20:22] != -0.5).any())


def test_sources_out_of_order_and_repeated(pkg, lib):
    src = kr.image_source(3, 50, 61, True, seed=45)
    order = [2, 0, 2, 1, 1, 0, 2]
    views = [(b, (n, 2 * n, 40 + 3 * n, 30 + 2 * n), n % 4, bool(n % 2), bool(n % 3 == 0)) for n, b in enumerate(order)]
    got = check_views(pkg, lib, "views sources_b3 u8->bf16", src, True, views, BF16, 42)
    rows = got.shape[0] // len(views)
    same = check_views(pkg, lib, "views sources_b3_single u8->bf16", src[2:3], True, [(0, *views[0][1:])], BF16, 42)
    assert torch.equal(got[:rows], same)                  # view 0 names image 2


@pytest.mark.parametrize("V", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1], ids=lambda v: f"V{v}")
def test_view_counts_across_record_chunks(pkg, lib, V):
    """One below, at and one above the 64 records of a launch, and two launches plus one: every view distinct, so a record
    read from the wrong chunk or written to the wrong rows shows."""
    src = kr.image_source(2, 40, 44, True, seed=46)
    views = [(n % 2, (n % 9, n % 7, 30 + n % 14, 28 + n % 11), n % 4, bool(n // 4 % 2), bool(n // 8 % 2)) for n in range(V)]
    check_views(pkg, lib, f"views count_V{V} u8->bf16", src, True, views, BF16, 14, 14, 640, True)


def test_grid_stride(pkg, lib):
    """V = 112 at S = 112: each launch of 64 views has 64 x 3 x 112 x 112 = 2 408 448 outputs, more than the 4096 x 256
    threads of the capped grid (small boxes up-sampled, so the taps stay two per axis)."""
    V, S = 112, 112
    assert CHUNK * 3 * S * S > 4096 * 256
    src = kr.image_source(2, 40, 44, True, seed=47)
    views = [(n % 2, (n % 9, n % 7, 20 + n % 14, 18 + n % 11), n % 4, bool(n // 4 % 2), bool(n // 8 % 2)) for n in range(V)]
    check_views(pkg, lib, "views grid_stride u8->bf16", src, True, views, BF16, S, patch=False)


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pkg, lib):
    B, Hs, Ws = 2, 60, 230
    src = kr.image_source(B, Hs, Ws, True, seed=48).to(DEV)
    out = out_buffer(2, 14, 14, 640, True, torch.bfloat16)
    good = (1, (3, 5, 45, 60), 1, True, True)

    def call(rec=(0, (0, 0, 50, 40), 0, False, False), src_=src, B_=B, V=2, out_=out.ptr, dt=BF16, S=14, Pp=14, Kp=640,
             std=0.5, tab="table"):
        t = table(pkg, [good, rec]) if tab == "table" else tab
        return lib.sgl_op_preprocess_views(P(src_), 1, B_, Hs, Ws, t, V, out_, dt, S, Pp, Kp, 1, 0.5, std, None, 0, stream())
    assert call(src_=None) == NULL and call(out_=None) == NULL and call(tab=None) == NULL
    assert call(V=0) == BAD_SHAPE and call(B_=0) == BAD_SHAPE and call(S=0) == BAD_SHAPE and call(std=0.0) == BAD_SHAPE
    assert call(Kp=587) == BAD_SHAPE and call(S=13) == BAD_SHAPE
    for rec in ((2, (0, 0, 50, 40), 0, 0, 0), (0, (-1, 0, 50, 40), 0, 0, 0), (0, (50, 0, 50, 40), 0, 0, 0),
                (0, (0, 0, 231, 40), 0, 0, 0), (0, (0, 0, 50, 61), 0, 0, 0), (0, (0, 0, 50, 40), 4, 0, 0),
                (0, (0, 0, 50, 40), 0, 2, 0), (0, (0, 0, 50, 40), 0, 0, 2)):
        assert call(rec=rec) == BAD_SHAPE, rec            # the first record is a good one: nothing of it is written either
    assert call(dt=2) == UNSUPPORTED and call(dt=4) == UNSUPPORTED
    assert call(rec=(0, (0, 0, 225, 40), 0, 0, 0)) == UNSUPPORTED            # 225 / 14 = 16.07
    assert call(rec=(0, (0, 0, 225, 40), 1, 0, 0)) == UNSUPPORTED            # the same extent turned onto the y axis
    torch.cuda.synchronize()
    untouched(out, "views refusals")


# ---- the Python surface ------------------------------------------------------------------------------------------
def app_like_views(pp, h, w):
    d = pp.detect_views(h, w)
    return d.views + [pp.View(0, (1, 2, w - 3, h - 1), turns=3, flip=True), pp.View(0, (0, 0, w, h), flip=True)]


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32src"])
def test_views_resize_normalize_against_the_reference(pkg, lib, u8):
    pp = pkg.preprocess
    h, w, S = 64, 97, 42
    src = kr.image_source(1, h, w, u8, seed=49)
    views = app_like_views(pp, h, w)
    assert len(views) == 44
    for dt in (torch.float32, torch.bfloat16):
        got = pp.views_resize_normalize(src.to(DEV), views, S, 0.5, 0.25, dtype=dt)
        assert got.shape == (44, 3, S, S) and got.dtype == dt
        ref, bound = vr.views_ref(src, u8, views, S, 14, 640, False, 0.5, 0.25, dt)
        within(got, ref, bound, f"views_resize_normalize {'u8' if u8 else 'f32'} {dt}")


@pytest.mark.parametrize("cfg_name", ["tiny", "hostile"])
def test_views_patch_operand_feeds_the_encoder_bitwise(pkg, lib, cfg_name):
    """model(patches=views_to_patch_operand(...)) == model(pixel_values=views_resize_normalize(...)) bit for bit under
    no_grad: one encoder batch of V rows without the fp32 pixel tensor or the im2col pass."""
    pp = pkg.preprocess
    cfg = pkg.get_config(cfg_name)
    S, Pp = cfg.image_size, cfg.patch_size
    h, w = 70, 97
    src = kr.image_source(1, h, w, True, seed=50).to(DEV)
    views = app_like_views(pp, h, w)
    for mode in ("bf16", "fp32"):
        model = build(pkg, cfg_name, 3, mode).eval()
        with torch.no_grad():
            op = pp.views_to_patch_operand(src, views, cfg, compute_dtype=mode)
            px = pp.views_resize_normalize(src, views, S)
            assert (op.batch, op.height, op.width) == (len(views), S, S)
            assert op.data.shape == (len(views) * (S // Pp) ** 2, (3 * Pp * Pp + 63) // 64 * 64)
            a, b = model(patches=op), model(pixel_values=px)
        assert a.pooler_output.shape[0] == len(views)
        assert torch.equal(a.pooler_output, b.pooler_output) and torch.equal(a.last_hidden_state, b.last_hidden_state)


def test_views_refuse_a_grad_requiring_source(pkg, lib):
    pp = pkg.preprocess
    cfg = pkg.get_config("tiny")
    src = kr.image_source(1, 40, 40, False, seed=51).to(DEV)
    x = src.clone().requires_grad_(True)
    views, _ = pp.multicrop_views(40, 40)
    for fn in (lambda t: pp.views_resize_normalize(t, views, 32), lambda t: pp.views_to_patch_operand(t, views, cfg, size=32)):
        with pytest.raises(RuntimeError, match="differentia"):
            fn(x)
        fn(src)
        with torch.no_grad():
            fn(x)
    with pytest.raises(ValueError, match="view 0"):
        pp.views_resize_normalize(src, [pp.View(0, (0, 0, 41, 40))], 32)
