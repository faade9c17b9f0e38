"""CPU (no GPU): the app's 24-D frequency / SRM feature vectors (sgl_op_freq_features, preprocess.views_freq_features).

* tests/freq_ref.py's integer gray plane equals PIL itself byte for byte (up-scale, down-scale, non-integer ratios, one
  axis already 256, 1 x 1, an off-origin box);
* its raw features match the values the reference app's own `extract_freq_vector` pipeline produced
  (tests/gen_golden_freq.py, tests/golden/freq/) within 1e-5 |v| + 1e-8: the reference computes in fp32, the restatement
  in integers and float64;
* `preprocess.freq_geometry()` equals the restatement's tables (the same torch calls written twice, so this guards
  against drift only; the independent pin of the geometry is the reference-made golden, whose gratings sit one bin to
  either side of each band and sector edge), with the 7 empty buckets, the DC pixel in no bucket and the atan2 == pi
  half-row in no sector;
* the new symbols are declared and exported (sgl_abi_version() stays 3), every documented refusal of the C call returns
  its code before the first HIP call (dummy pointers, no launch), and every documented ValueError is raised.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import freq_ref as fr

OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE, NULL = 0, -1, -2, -3, -5
D = 0x7F0000001000          # an aligned dummy device pointer, never dereferenced
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freq")
with open(os.path.join(GOLDEN, "cases.json")) as _f:
    DOC = json.load(_f)
SOURCES = np.load(os.path.join(GOLDEN, "sources.npz"))
EXPECTED = np.load(os.path.join(GOLDEN, "expected.npz"))
CASES = list(DOC["cases"])


# ---- gray plane against PIL itself -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 64), (97, 31), (300, 517), (256, 100), (700, 256), (33, 1031), (1, 1)],
                         ids=lambda v: str(v))
def test_gray_plane_equals_pil(w, h):
    img = np.random.default_rng(w * 4099 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img).convert("L").resize((256, 256), Image.BICUBIC))
    got = fr.gray256(img, (0, 0, w, h))
    assert got.dtype == np.uint8 and int((got != want).sum()) == 0


def test_gray_plane_of_an_off_origin_box_equals_pil():
    img = np.random.default_rng(7).integers(0, 256, (211, 173, 3), dtype=np.uint8)
    box = (19, 33, 160, 170)
    want = np.asarray(Image.fromarray(img).crop(box).convert("L").resize((256, 256), Image.BICUBIC))
    assert int((fr.gray256(img, box) != want).sum()) == 0


# ---- the restatement against the reference's own numbers ---------------------------------------------------------
def test_golden_holds_the_inputs_of_the_issue():
    assert CASES == ["noise", "smooth_noise", "black", "grating_r27", "grating_r28", "grating_r81_in", "grating_r81_out",
                     "grating_axis", "grating_diag", "multicrop_130x97"]
    assert all(max(SOURCES[c].shape) <= 160 for c in CASES)
    assert SOURCES["multicrop_130x97"].shape == (97, 130, 3) and len(DOC["cases"]["multicrop_130x97"]["boxes"]) == 9
    assert sum(1 for k in EXPECTED.files if k.endswith(".gray")) <= 4
    assert max(DOC["fp32_reference_vs_freq_ref_in_tolerances"].values()) <= 1.0      # recorded at generation time


@pytest.mark.parametrize("case", CASES)
def test_raw_features_match_the_reference_golden(case):
    img, info = SOURCES[case], DOC["cases"][case]
    for n, box in enumerate(info["boxes"]):
        plane = fr.gray256(img, box)
        assert hashlib.sha256(plane.tobytes()).hexdigest() == info["gray_sha256"][n], f"{case}[{n}]: gray plane"
        if n == 0 and f"{case}.gray" in EXPECTED.files:
            assert np.array_equal(plane, EXPECTED[f"{case}.gray"])
        got, want = fr.raw_features(plane), EXPECTED[f"{case}.raw"][n]
        ratio = np.abs(got - want) / (1e-5 * np.abs(got) + 1e-8)
        worst = int(ratio.argmax())
        print(f"RATIO freq_ref vs reference {case}[{n}]: {ratio.max():.4f} at {fr.NAMES[worst]}")
        assert ratio.max() <= 1.0, f"{case}[{n}] {fr.NAMES[worst]}: {got[worst]!r} vs {want[worst]!r}"
        std = fr.standardize(want.astype(np.float32))
        assert np.abs(std - EXPECTED[f"{case}.std"][n]).max() <= 1e-5, f"{case}[{n}]: standardised vector"


# ---- geometry ----------------------------------------------------------------------------------------------------
def test_freq_geometry_equals_the_restatement(pkg):
    mine, ref = pkg.preprocess.freq_geometry(), fr.geometry()
    assert len(mine) == 3
    for got, want, name in zip(mine, ref, ("band", "bucket", "sector")):
        assert got.dtype == torch.uint8 and tuple(got.shape) == (256, 256), name
        assert torch.equal(got, want), name
    band, bucket, sector = mine
    assert bucket[128, 128] == 255 and int((bucket == 255).sum()) == 1          # the DC pixel lands in bucket -1
    counts = torch.bincount(bucket.flatten().long(), minlength=256)[:39]
    assert int((counts == 0).sum()) == 7                                         # empty buckets count as 0 in the slope
    none = sector == 255
    assert int(none.sum()) == 128 and bool(none[128, :128].all())                # atan2 == pi: x < cx on the centre row
    assert sorted(torch.unique(band).tolist()) == [0, 1, 2] and band[128, 128] == 0
    assert pkg.preprocess.freq_geometry()[0] is band                             # built once, owned by the cache


def test_detect_views_lists_the_frequency_windows(pkg):
    d = pkg.preprocess.detect_views(97, 130)
    assert d.freq == list(range(9)) + list(range(10, 42, 2)) and len(d.freq) == 25
    assert all(d.views[n].turns == 0 for n in d.freq)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------
def test_symbols_exist_and_argument_errors_return_before_any_launch(pkg, hiplib):
    """Fails on the parent: the symbols are neither declared nor exported there."""
    lib = hiplib
    declared = pkg.lib.declared_symbols()
    for s in ("sgl_op_freq_features", "sgl_op_freq_features_scratch_bytes"):
        assert s in declared, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.sgl_abi_version() == 3                               # new symbols only
    View = pkg.lib.SglView
    Hs, Ws = 60, 5000
    need = lib.sgl_op_freq_features_scratch_bytes(2, Hs, Ws)
    assert need > 2 * (65536 + 256 * 256 * 8)                       # at least the gray plane and the row-pass spectrum
    assert lib.sgl_op_freq_features_scratch_bytes(0, Hs, Ws) == 0
    assert lib.sgl_op_freq_features_scratch_bytes(65, Hs, Ws) == lib.sgl_op_freq_features_scratch_bytes(64, Hs, Ws)

    def call(src=D, B=2, Hs_=Hs, Ws_=Ws, rec=(0, 0, 0, 50, 40, 0, 0, 0), V=2, geom=D, out=D, views="table", scratch=D,
             nbytes=need):
        tab = (View * 2)(View(1, 3, 5, 45, 60, 0, 0, 0), View(*rec))     # a good record, then the one under test
        return lib.sgl_op_freq_features(src, B, Hs_, Ws_, tab if views == "table" else views, V, geom, out, 1, None,
                                        scratch, nbytes, None)
    assert call(nbytes=need - 1) == WORKSPACE                       # passes every other rule: the last check answers
    assert call(src=None) == NULL and call(out=None) == NULL and call(views=None) == NULL and call(geom=None) == NULL
    assert call(src=None, V=0) == NULL                              # pointers are checked first
    for over in (dict(V=0), dict(V=-1), dict(B=0), dict(Hs_=0), dict(Ws_=0),
                 dict(rec=(2, 0, 0, 50, 40, 0, 0, 0)), dict(rec=(-1, 0, 0, 50, 40, 0, 0, 0)),      # src outside the batch
                 dict(rec=(0, 10, 0, 10, 40, 0, 0, 0)), dict(rec=(0, 0, 40, 50, 40, 0, 0, 0)),      # empty box
                 dict(rec=(0, -1, 0, 50, 40, 0, 0, 0)), dict(rec=(0, 0, 0, Ws + 1, 40, 0, 0, 0)),   # outside the source
                 dict(rec=(0, 0, 0, 50, Hs + 1, 0, 0, 0))):
        assert call(**over) == BAD_SHAPE, over
    for over in (dict(rec=(0, 0, 0, 50, 40, 1, 0, 0)), dict(rec=(0, 0, 0, 50, 40, 0, 1, 0)),
                 dict(rec=(0, 0, 0, 50, 40, 0, 0, 1)), dict(rec=(0, 0, 0, 4097, 40, 0, 0, 0))):
        assert call(**over) == UNSUPPORTED, over
    assert call(rec=(0, 0, 0, 4096, 40, 0, 0, 0), nbytes=0) == WORKSPACE      # 4096 is inside the cap
    assert call(rec=(0, 0, 0, 50, 40, 1, 0, 0), nbytes=0) == UNSUPPORTED      # before the workspace check
    assert call(scratch=None) == NULL
    assert call(scratch=D + 8) == UNSUPPORTED                       # double2 accesses: 16-byte aligned scratch only
    assert call(scratch=D + 8, nbytes=0) == UNSUPPORTED             # before the workspace check


def test_python_entry_refuses_with_value_errors(pkg):
    pp = pkg.preprocess
    u8 = torch.zeros(1, 40, 5000, 3, dtype=torch.uint8)
    box = (0, 0, 30, 20)
    with pytest.raises(ValueError, match="uint8"):
        pp.views_freq_features(torch.zeros(1, 3, 40, 50), [pp.View(0, box)])
    with pytest.raises(ValueError, match="detach"):
        pp.views_freq_features(torch.zeros(1, 3, 40, 50, requires_grad=True), [pp.View(0, box)])
    for bad in (dict(turns=1), dict(turns=2, keep_canvas=True), dict(flip=True)):
        with pytest.raises(ValueError, match="views_resize_normalize"):
            pp.views_freq_features(u8, [pp.View(0, box), pp.View(0, box, **bad)])
    with pytest.raises(ValueError, match="4096"):
        pp.views_freq_features(u8, [pp.View(0, (0, 0, 4097, 20))])
    with pytest.raises(ValueError, match="outside"):
        pp.views_freq_features(u8, [pp.View(0, (0, 0, 30, 41))])
    with pytest.raises(ValueError, match="NHWC"):
        pp.views_freq_features(torch.zeros(1, 3, 40, 50, dtype=torch.uint8), [pp.View(0, box)])


def test_core_signals_batched_still_builds_no_graph(pkg):
    """`app_freq_logits` sits next to `core_signals_batched`: both run under no_grad, a trainable fusion head included."""
    H = pkg.heads
    fusion = torch.nn.Linear(2, 1)
    out = H.core_signals_batched(torch.zeros(1, 9), torch.full((9,), 1 / 9), torch.zeros(1, 9), torch.zeros(1), fusion,
                                 H.CoralCalibrator())
    assert not out["z"].requires_grad and not out["p_fake_raw"].requires_grad


def test_an_fp32_transform_could_not_meet_the_caps():
    """Why the kernel transforms in fp64: the same propagation with an fp32 FFT's per-bin error (16 * 2^-24 * rms|F|, one
    unit per pass) puts the bound of the up-scaled gratings above the caps the contract sets, the fp64 one far below."""
    for case, feature, cap_of in (("grating_r27", 6, lambda v: 2e-3), ("grating_r28", 4, lambda v: 1e-4 * abs(v) + 1e-8)):
        plane = fr.gray256(SOURCES[case], DOC["cases"][case]["boxes"][0])
        cap = cap_of(fr.raw_features(plane)[feature])
        b32, b64 = fr.raw_bound(plane, "fp32")[feature], fr.raw_bound(plane)[feature]
        print(f"RATIO bound/cap {case} {fr.NAMES[feature]}: fp32 transform {b32 / cap:.2f}, fp64 transform {b64 / cap:.4f}")
        assert b32 > cap and b64 < 0.25 * cap

