"""CPU (no GPU): the app's test-time views (preprocess.View and its builders, sgl_op_preprocess_views).

* the view builders reproduce tests/golden/app_views.json, the boxes and weights the reference app's own
  `make_multicrops` / `compute_patch_grid` produced on a box-recording stub image (tests/gen_golden_views.py);
* `detect_views` lays the families out as documented; `view_table` refuses what the C side refuses;
* the new symbols are declared and exported (sgl_abi_version() stays 3) and every documented refusal of the C call
  returns its code before the first HIP call (dummy pointers, no launch: the method of tests/test_preprocess_bwd_host.py);
* the float64 reference (tests/views_ref.py) is held against PIL itself: the `keep_canvas` orientation equals
  `Image.rotate(90 k)` exactly, and a whole uint8 view equals `crop -> rotate -> resize(BILINEAR)` within 1.05 / 255.
"""
import ctypes as C
import json
import os

import pytest
import torch

import views_ref as vr

OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE, NULL = 0, -1, -2, -3, -5
D = 0x7F0000001000          # a 16-byte aligned dummy device pointer, never dereferenced
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "app_views.json")
with open(GOLDEN) as _f:
    APP = json.load(_f)
CASES = APP["cases"]
CASE_IDS = [f"{c['w']}x{c['h']}" for c in CASES]


# ---- the builders against the reference app's recorded boxes -----------------------------------------------------
def test_golden_holds_the_sizes_of_the_issue():
    assert [(c["w"], c["h"]) for c in CASES] == [(64, 64), (97, 64), (65, 130), (640, 427), (1031, 777), (2048, 1365), (3, 9)]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_multicrop_views_reproduce_the_app(pkg, case):
    pp = pkg.preprocess
    w, h = case["w"], case["h"]
    views, weights = pp.multicrop_views(h, w, src=2)
    assert weights.dtype == torch.float32 and weights.tolist() == case["weights"]     # the fp32 values, exactly
    assert len(views) == case["num_crops"]
    assert all(v.src == 2 and v.turns == 0 and not v.keep_canvas and not v.flip for v in views)
    if case["multicrop_fallback_resize"] is None:
        assert [list(v.box) for v in views] == case["multicrop_boxes"] and len(views) == 9
    else:                                                  # w < 4 or h < 4: the app resizes the whole image, crops nothing
        assert case["multicrop_boxes"] == [] and [list(v.box) for v in views] == [[0, 0, w, h]]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_patch_grid_views_reproduce_the_app(pkg, case):
    pp = pkg.preprocess
    w, h = case["w"], case["h"]
    k = APP["constants"]
    cells = pp.patch_grid_views(h, w, k["PATCH_GRID_ROWS"], k["PATCH_GRID_COLS"], src=1, min_side=k["MIN_SIDE"])
    assert cells == pp.patch_grid_views(h, w, src=1)                                   # the defaults are the app's
    if case["grid"] is None:
        assert cells == []
        return
    assert (case["grid"]["rows"], case["grid"]["cols"]) == (4, 4)
    assert [None if c is None else list(c.box) for c in cells] == case["grid"]["cells"]
    assert all(c is None or (c.src == 1 and c.turns == 0 and not c.flip) for c in cells)


def test_patch_grid_views_mark_empty_cells(pkg):
    """8-pixel minimum cells on a 20-wide image leave the fourth column empty: 0-8, 8-16, 16-20 (clipped), then nothing."""
    cells = pkg.preprocess.patch_grid_views(40, 20, 2, 4, min_side=0)
    assert [None if c is None else c.box for c in cells] == [
        (0, 0, 8, 20), (8, 0, 16, 20), (16, 0, 20, 20), None, (0, 20, 8, 40), (8, 20, 16, 40), (16, 20, 20, 40), None]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_detect_views_layout(pkg, case):
    pp = pkg.preprocess
    w, h = case["w"], case["h"]
    d = pp.detect_views(h, w)
    crops, weights = pp.multicrop_views(h, w)
    cells = [c for c in pp.patch_grid_views(h, w) if c is not None]
    assert len(d.views) == len(crops) + 1 + 2 * len(cells)
    if case["grid"] is not None and case["multicrop_fallback_resize"] is None:
        assert len(d.views) == 42 and d.rot == 9 and d.grid_start == 10               # 9 + 1 + 2 * 16
    assert d.views[d.crops] == crops and torch.equal(d.weights, weights)
    assert d.rot == len(crops) and d.views[d.rot] == pp.View(0, (0, 0, w, h), turns=1, keep_canvas=True)
    assert d.views[d.rot] == pp.rotated_view((0, 0, w, h))
    assert d.views[d.grid] == cells
    assert d.views[d.grid_rot] == [pp.rotated_view(c.box) for c in cells]
    assert len(d.cells) == len(cells)
    for n, (r, c) in enumerate(d.cells):                                                # cell n is followed by its turn
        assert d.views[d.grid_start + 2 * n] == pp.patch_grid_views(h, w)[r * 4 + c]
        assert d.views[d.grid_start + 2 * n + 1].box == d.views[d.grid_start + 2 * n].box
    pp.view_table(d.views, 1, h, w)                                                    # every record is a legal one


def test_detect_views_skips_empty_cells_and_names_the_kept_ones(pkg):
    pp = pkg.preprocess
    d = pp.detect_views(64, 64, grid=(2, 9))               # pw = max(8, 64 // 9) = 8: the ninth column starts at 64
    assert len(d.cells) == 16 and (0, 8) not in d.cells and (1, 7) in d.cells
    assert len(d.views) == 10 + 2 * 16


# ---- view_table --------------------------------------------------------------------------------------------------
def test_view_table_packs_records(pkg):
    pp = pkg.preprocess
    tab = pp.view_table([pp.View(1, (2, 3, 10, 9), 3, True, True), pp.View(0, (0, 0, 20, 12))], 2, 12, 20)
    assert C.sizeof(tab) == 64 and C.sizeof(pkg.lib.SglView) == 32
    assert [getattr(tab[0], n) for n, _ in pkg.lib.SglView._fields_] == [1, 2, 3, 10, 9, 3, 1, 1]
    assert [getattr(tab[1], n) for n, _ in pkg.lib.SglView._fields_] == [0, 0, 0, 20, 12, 0, 0, 0]
    assert pp.View(0, (0, 0, 8, 5), 1).oriented_hw() == (8, 5) and pp.View(0, (0, 0, 8, 5), 1, True).oriented_hw() == (5, 8)


BAD_RECORDS = [
    ("src_low", dict(src=-1)), ("src_high", dict(src=2)), ("x0_neg", dict(box=(-1, 0, 5, 5))),
    ("empty_x", dict(box=(5, 0, 5, 5))), ("reversed_y", dict(box=(0, 6, 5, 5))), ("x1_past", dict(box=(0, 0, 21, 5))),
    ("y1_past", dict(box=(0, 0, 5, 13))), ("turns_4", dict(turns=4)), ("turns_neg", dict(turns=-1)),
    ("keep_2", dict(keep_canvas=2)), ("flip_2", dict(flip=2)), ("float_box", dict(box=(0.5, 0, 5, 5))),
]


@pytest.mark.parametrize("name,over", BAD_RECORDS, ids=[b[0] for b in BAD_RECORDS])
def test_view_table_refuses_bad_records(pkg, name, over):
    pp = pkg.preprocess
    good = dict(src=0, box=(0, 0, 20, 12), turns=0, keep_canvas=False, flip=False)
    pp.view_table([pp.View(**good)], 2, 12, 20)
    with pytest.raises(ValueError, match="view 1"):
        pp.view_table([pp.View(**good), pp.View(**{**good, **over})], 2, 12, 20)


def test_view_table_refuses_an_empty_list_and_foreign_records(pkg):
    pp = pkg.preprocess
    with pytest.raises(ValueError):
        pp.view_table([], 1, 8, 8)
    with pytest.raises(ValueError, match="not a View"):
        pp.view_table([(0, (0, 0, 8, 8))], 1, 8, 8)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------
def test_symbols_exist_and_argument_errors_return_before_any_launch(pkg, hiplib):
    """This is the test that fails on the parent: the symbols are neither declared nor exported there."""
    lib = hiplib
    declared = pkg.lib.declared_symbols()
    for s in ("sgl_op_preprocess_views", "sgl_op_preprocess_views_scratch_bytes"):
        assert s in declared, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.sgl_abi_version() == 3                               # new symbols only
    need = lib.sgl_op_preprocess_views_scratch_bytes(42, 384)
    assert need == 0                                                # the records travel in the kernel arguments
    View = pkg.lib.SglView
    Hs, Ws = 60, 700

    def call(src=D, B=2, Hs_=Hs, Ws_=Ws, rec=(0, 0, 0, 50, 40, 0, 0, 0), V=2, out=D, dt=1, S=42, P=14, Kp=640, patch=1,
             std=0.5, views="table", scratch=None, nbytes=0):
        tab = (View * 2)(View(1, 3, 5, 45, 60, 1, 1, 1), View(*rec))     # a good record, then the one under test
        return lib.sgl_op_preprocess_views(src, 1, B, Hs_, Ws_, tab if views == "table" else views, V, out, dt, S, P, Kp,
                                           patch, 0.5, std, scratch, nbytes, None)
    assert call(rec=(0, 0, 0, 673, 60, 0, 0, 0)) == UNSUPPORTED    # passes every shape rule: the next check answers
    assert call(src=None) == NULL and call(out=None) == NULL and call(views=None) == NULL
    assert call(src=None, V=0) == NULL                              # pointers are checked first
    for over in (dict(V=0), dict(V=-1), dict(B=0), dict(Hs_=0), dict(Ws_=0), dict(S=0), dict(std=0.0),
                 dict(Kp=587), dict(S=13), dict(P=0)):
        assert call(**over) == BAD_SHAPE, over
    for rec in ((2, 0, 0, 50, 40, 0, 0, 0), (-1, 0, 0, 50, 40, 0, 0, 0),          # src outside the batch
                (0, -1, 0, 50, 40, 0, 0, 0), (0, 0, -1, 50, 40, 0, 0, 0),         # negative corner
                (0, 50, 0, 50, 40, 0, 0, 0), (0, 0, 40, 50, 40, 0, 0, 0),         # empty
                (0, 51, 0, 50, 40, 0, 0, 0), (0, 0, 41, 50, 40, 0, 0, 0),         # reversed
                (0, 0, 0, 701, 40, 0, 0, 0), (0, 0, 0, 50, 61, 0, 0, 0),          # past the source
                (0, 0, 0, 50, 40, 4, 0, 0), (0, 0, 0, 50, 40, -1, 0, 0),          # turns
                (0, 0, 0, 50, 40, 0, 2, 0), (0, 0, 0, 50, 40, 0, -1, 0),          # keep_canvas
                (0, 0, 0, 50, 40, 0, 0, 2), (0, 0, 0, 50, 40, 0, 0, -1)):         # flip
        assert call(rec=rec) == BAD_SHAPE, rec
        assert call(rec=rec, dt=2) == BAD_SHAPE, rec                # a bad record is reported before a bad dtype
    assert call(dt=2) == UNSUPPORTED and call(dt=4) == UNSUPPORTED and call(dt=5) == UNSUPPORTED
    assert call(rec=(0, 0, 0, 673, 60, 0, 0, 0)) == UNSUPPORTED    # 673 > 16 * 42 along x
    assert call(rec=(0, 0, 0, 673, 60, 1, 1, 0)) == UNSUPPORTED    # the kept canvas keeps the width
    assert call(rec=(0, 0, 0, 673, 60, 3, 0, 0)) == UNSUPPORTED    # an exact turn moves it to the y axis
    assert call(rec=(0, 0, 0, 673, 60, 0, 0, 0), patch=0, P=0, Kp=0) == UNSUPPORTED   # NCHW reads neither P nor Kp
    assert call(rec=(0, 0, 0, 673, 60, 0, 0, 0), S=13, patch=0) == UNSUPPORTED        # and S < P is no error there
    # SGL_ERR_WORKSPACE cannot be provoked: the design needs 0 bytes of scratch, and no size is below that


# ---- the reference against PIL -----------------------------------------------------------------------------------
def _bytes(h, w, seed):
    return torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("hw", [(5, 8), (8, 5), (6, 10), (10, 6), (7, 7), (6, 6), (64, 97), (33, 16), (1, 4), (4, 1)],
                         ids=lambda s: f"{s[1]}x{s[0]}")
def test_keep_canvas_orientation_is_pil_rotate(hw, k):
    """w - h even, odd and zero, both signs; the 8 x 5 example of include/siglip_hip.h among them."""
    Image = pytest.importorskip("PIL.Image")
    np = pytest.importorskip("numpy")
    h, w = hw
    img = _bytes(h, w, seed=h * 31 + w)
    want = torch.from_numpy(np.asarray(Image.fromarray(img.numpy()).rotate(90 * k)).copy())
    got = vr.orient(img.permute(2, 0, 1), k, True, False).permute(1, 2, 0)
    assert got.shape == want.shape == (h, w, 3)
    assert torch.equal(got, want)
    if (h, w, k) == (5, 8, 1):                             # O[y][x] = C[x - 1][6 - y] for x in 1..5, zero for x in {0, 6, 7}
        for y in range(5):
            for x in range(8):
                assert torch.equal(got[y, x], img[x - 1, 6 - y] if 1 <= x <= 5 else torch.zeros(3, dtype=torch.uint8))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_exact_turns_are_pil_transpose_and_expand(k):
    Image = pytest.importorskip("PIL.Image")
    np = pytest.importorskip("numpy")
    img = _bytes(5, 8, seed=k)
    pil = Image.fromarray(img.numpy())
    t = pil
    for _ in range(k):
        t = t.transpose(Image.ROTATE_90)
    got = vr.orient(img.permute(2, 0, 1), k, False, False).permute(1, 2, 0)
    assert torch.equal(got, torch.from_numpy(np.asarray(t).copy()))
    assert torch.equal(got, torch.from_numpy(np.asarray(pil.rotate(90 * k, expand=True)).copy()))
    assert torch.equal(got, torch.from_numpy(np.rot90(img.numpy(), k).copy()))
    flipped = vr.orient(img.permute(2, 0, 1), k, False, True).permute(1, 2, 0)
    assert torch.equal(flipped, torch.from_numpy(np.asarray(t.transpose(Image.FLIP_LEFT_RIGHT)).copy()))


@pytest.mark.parametrize("rotate", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("S", [28, 64])
@pytest.mark.parametrize("wh", [(97, 64), (640, 427)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_uint8_view_is_pil_crop_rotate_resize_within_1p05_levels(pkg, wh, S, rotate):
    """Before normalisation, every one of the 9 crops: |ref - PIL / 255| <= 1.05 / 255.  PIL stores 8 bits after each of
    its two resize passes (half a level each) and quantises its coefficients to 22 bits; this path does neither: the
    stated deviation.  Worst measured on random bytes: 1.00 level."""
    Image = pytest.importorskip("PIL.Image")
    np = pytest.importorskip("numpy")
    pp = pkg.preprocess
    w, h = wh
    src = _bytes(h, w, seed=w + S)[None]
    pil = Image.fromarray(src[0].numpy())
    views, _ = pp.multicrop_views(h, w)
    if rotate:
        views = [pp.rotated_view(v.box) for v in views]
    ref, _ = vr.views_resized_ref(src, True, views, S)
    worst = 0.0
    for n, v in enumerate(views):
        c = pil.crop(v.box)
        if rotate:
            c = c.rotate(90, expand=False)
        want = torch.from_numpy(np.asarray(c.resize((S, S), Image.BILINEAR)).copy()).permute(2, 0, 1).double() / 255.0
        worst = max(worst, (ref[n] - want).abs().max().item() * 255.0)
    print(f"PILERR {w}x{h} S {S} {'rotated' if rotate else 'plain'}: worst {worst:.4f} levels")
    assert worst <= 1.05
