"""GPU: sgl_op_freq_features, the app's 24-D frequency / SRM vector of V windows in one pass, through the C ABI and up to
`heads.app_freq_logits`.

The gray plane is compared bit for bit with tests/freq_ref.py (pinned to PIL on the CPU in
tests/test_freq_features_host.py); every feature is held to the bound freq_ref derives from the float64 reference alone,
and the test first asserts that this bound itself stays under the caps of the feature's contract: 1e-4 |ref| + 1e-8 per
raw feature, 2e-3 absolute for the entropy, 1e-3 for the standardised vector.  Every call runs on guarded outputs and a
poisoned, guarded scratch; each case prints its worst err / bound as a RATIO line before it asserts.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import freq_ref as fr
from test_kernel_edges_gpu import DEV, Guarded, P, lib, ok, stream  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "freq", "cases.json")) as _f:
    DOC = json.load(_f)
SOURCES = np.load(os.path.join(GOLDEN, "freq", "sources.npz"))
EXPECTED = np.load(os.path.join(GOLDEN, "freq", "expected.npz"))
CASES = list(DOC["cases"])
GUARD = 4096                 # bytes either side of the byte buffers (keeps the scratch's alignment)


class GuardedBytes:
    """`n` bytes between two sentinel bands; the body holds `fill`."""

    def __init__(self, n, fill):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), 0xA5, device=DEV, dtype=torch.uint8)
        self.body = self.buf[GUARD:GUARD + n]
        self.body.fill_(fill)
        self.ptr = self.body.data_ptr()

    def check(self, what):
        assert bool((self.buf[:GUARD] == 0xA5).all()), f"{what}: bytes BEFORE the buffer were written"
        assert bool((self.buf[GUARD + self.n:] == 0xA5).all()), f"{what}: bytes AFTER the buffer were written"


def run(pkg, lib, what, src, views, standardize, poison=0xCD, on_stream=None):
    """One guarded call: (out (V, 24) float32 cpu, gray (V, 256, 256) uint8 cpu).  `views`: (src index, box) pairs."""
    src_d = torch.as_tensor(src).to(DEV)
    B, Hs, Ws = src_d.shape[:3]
    V = len(views)
    tab = (pkg.lib.SglView * V)(*(pkg.lib.SglView(b, *box, 0, 0, 0) for b, box in views))
    out = Guarded(V, 24, 24, torch.float32)
    gray = GuardedBytes(V * 65536, 0x3C)
    nbytes = lib.sgl_op_freq_features_scratch_bytes(V, Hs, Ws)
    scratch = GuardedBytes(nbytes, poison)
    geom = pkg.preprocess.freq_geometry_on(torch.device(DEV, torch.cuda.current_device()))
    ok(lib.sgl_op_freq_features(P(src_d), B, Hs, Ws, tab, V, P(geom), out.ptr, int(standardize), gray.ptr, scratch.ptr,
                                nbytes, on_stream if on_stream is not None else stream()))
    torch.cuda.synchronize()
    out.check(what)
    gray.check(what + " gray_out")
    scratch.check(what + " scratch")
    return out.got().cpu().clone(), gray.body.view(V, 256, 256).cpu().clone()


@functools.lru_cache(maxsize=None)
def reference(case):
    """Per window of a golden case: (plane, raw, raw bound, standardised, its bound), computed once."""
    img = SOURCES[case]
    rows = []
    for box in DOC["cases"][case]["boxes"]:
        plane = fr.gray256(img, tuple(box))
        raw, bound = fr.raw_features(plane), fr.raw_bound(plane)
        rows.append((plane, raw, bound, fr.standardize(raw), fr.std_bound(raw, bound)))
    return rows


def views_of(case):
    return [(0, tuple(b)) for b in DOC["cases"][case]["boxes"]]


# ---- gray plane, bit for bit -------------------------------------------------------------------------------------
WINDOWS = [("identity_256", 256, 256), ("upscale_5x7", 5, 7), ("upscale_1x1", 1, 1), ("nonint_down_300x517", 300, 517),
           ("one_axis_skipped_256x100", 256, 100), ("taps65_4096x8", 4096, 8)]


@pytest.mark.parametrize("name,w,h", WINDOWS, ids=[c[0] for c in WINDOWS])
def test_gray_plane_bit_equal(pkg, lib, name, w, h):
    img = np.random.default_rng(w * 8191 + h).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    _, gray = run(pkg, lib, f"freq gray {name}", img, [(0, (0, 0, w, h))], False)
    want = fr.gray256(img[0], (0, 0, w, h))
    diff = int((gray[0].numpy() != want).sum())
    print(f"RATIO freq gray {name}: {diff} differing bytes")
    assert diff == 0


def test_gray_plane_reads_nothing_outside_the_box(pkg, lib):
    """An off-origin box in image 1 of 2; everything round the box holds the opposite extreme, so one tap past the edge
    would show.  The reference is the plane of the cropped copy alone."""
    rng = np.random.default_rng(5)
    x0, y0, x1, y1 = 37, 21, 150, 190
    img = np.full((2, 230, 201, 3), 255, dtype=np.uint8)
    img[1, y0:y1, x0:x1] = rng.integers(0, 48, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    img[0] = rng.integers(0, 256, img[0].shape, dtype=np.uint8)
    _, gray = run(pkg, lib, "freq gray off_origin", img, [(1, (x0, y0, x1, y1))], False)
    want = fr.gray256(np.ascontiguousarray(img[1, y0:y1, x0:x1]), (0, 0, x1 - x0, y1 - y0))
    assert int((gray[0].numpy() != want).sum()) == 0
    assert int(want.max()) < 64                                     # the 255s outside would have lifted the border


# ---- features against the float64 reference, on every golden input -----------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_features_within_the_derived_bound(pkg, lib, case):
    ref = reference(case)
    src = SOURCES[case][None]
    raw, gray = run(pkg, lib, f"freq raw {case}", src, views_of(case), False)
    std, _ = run(pkg, lib, f"freq std {case}", src, views_of(case), True, poison=0x00)
    for n, (plane, want, bound, want_std, bound_std) in enumerate(ref):
        assert np.array_equal(gray[n].numpy(), plane), f"{case}[{n}]: gray plane"
        cap = 1e-4 * np.abs(want) + 1e-8
        cap[6] = 2e-3
        assert bool((bound <= cap).all()), f"{case}[{n}]: bound above its cap at {fr.NAMES[int((bound / cap).argmax())]}"
        assert float(bound_std.max()) <= 1e-3, f"{case}[{n}]: standardised bound {bound_std.max()}"
        err = np.abs(raw[n].double().numpy() - want)
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
        worst = int(ratio.argmax())
        print(f"RATIO freq raw {case}[{n}]: {ratio.max():.4f} at {fr.NAMES[worst]} (bound/cap {float((bound / cap).max()):.4f})")
        assert bool(np.isfinite(raw[n].numpy()).all()) and ratio.max() <= 1.0, \
            f"{case}[{n}] {fr.NAMES[worst]}: got {raw[n][worst].item()!r}, want {want[worst]!r} +- {bound[worst]!r}"
        err = np.abs(std[n].double().numpy() - want_std)
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound_std, 1e-300))
        worst = int(ratio.argmax())
        print(f"RATIO freq std {case}[{n}]: {ratio.max():.4f} at {fr.NAMES[worst]}")
        assert bool(np.isfinite(std[n].numpy()).all()) and ratio.max() <= 1.0, \
            f"{case}[{n}] standardised {fr.NAMES[worst]}: got {std[n][worst].item()!r}, want {want_std[worst]!r}"


# ---- launch batches, determinism, streams ------------------------------------------------------------------------
def test_one_view_and_two_launch_batches(pkg, lib):
    """V = 65 is two launch groups (64 + 1); views repeat with period 3, so equal windows must give equal bits in either
    group and in every scratch slot.  V = 1 equals them too."""
    src = SOURCES["multicrop_130x97"][None]
    boxes = views_of("multicrop_130x97")[:3]
    views = [boxes[n % 3] for n in range(65)]
    out, gray = run(pkg, lib, "freq V65", src, views, True)
    for n in range(3, 65):
        assert torch.equal(out[n], out[n % 3]) and torch.equal(gray[n], gray[n % 3]), f"view {n}"
    one, gray1 = run(pkg, lib, "freq V1", src, boxes[:1], True)
    assert torch.equal(one[0], out[0]) and torch.equal(gray1[0], gray[0])
    assert not torch.equal(out[0], out[1])


def test_two_calls_give_the_same_bits(pkg, lib):
    src = SOURCES["noise"][None]
    a, _ = run(pkg, lib, "freq twice a", src, views_of("noise") * 5, False, poison=0xCD)
    b, _ = run(pkg, lib, "freq twice b", src, views_of("noise") * 5, False, poison=0x11)
    assert torch.equal(a, b)


def test_on_a_side_stream(pkg, lib):
    src = SOURCES["smooth_noise"][None]
    want, want_gray = run(pkg, lib, "freq default stream", src, views_of("smooth_noise"), True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, gray = run(pkg, lib, "freq side stream", src, views_of("smooth_noise"), True, on_stream=side.cuda_stream)
    assert torch.equal(got, want) and torch.equal(gray, want_gray)


# ---- the Python entries ------------------------------------------------------------------------------------------
def test_views_freq_features_equals_the_c_call(pkg, lib):
    pp = pkg.preprocess
    src = SOURCES["multicrop_130x97"][None]
    views, _ = pp.multicrop_views(97, 130)
    want, want_gray = run(pkg, lib, "freq python", src, views_of("multicrop_130x97"), True)
    got, gray = pp.views_freq_features(torch.from_numpy(src).to(DEV), views, return_gray=True)
    assert got.shape == (9, 24) and got.dtype == torch.float32 and gray.shape == (9, 256, 256) and gray.dtype == torch.uint8
    assert torch.equal(got.cpu(), want) and torch.equal(gray.cpu(), want_gray)
    raw = pp.views_freq_features(torch.from_numpy(src).to(DEV), views, standardize=False)
    assert abs(float(raw[0, 6]) - reference("multicrop_130x97")[0][1][6]) <= 2e-3


def test_app_freq_logits_on_the_130x97_golden(pkg, lib):
    """The crops' logits against FreqMLPApp(jitter=False) on the vectors the reference app itself produced, the cells'
    against the same MLP on freq_ref's vectors.  Bound: the MLP's gradient at the reference vector times the input's
    bound (the standardised bound, plus 1e-5 for the reference's own fp32 route on the crops), doubled for the
    curvature, plus 1e-5 for the fp32 forward."""
    from safetensors.torch import load_file
    pp, H = pkg.preprocess, pkg.heads
    img = SOURCES["multicrop_130x97"]
    d = pp.detect_views(97, 130)
    assert len(d.freq) == 25 and [list(d.views[n].box) for n in d.freq[:9]] == DOC["cases"]["multicrop_130x97"]["boxes"]
    mlp = H.FreqMLPApp()
    mlp.load_state_dict(load_file(os.path.join(GOLDEN, "ref_siglip", "freq_mlp.safetensors")))
    vecs, slack = [], []
    for n, (_, _, _, _, bound_std) in enumerate(reference("multicrop_130x97")):
        vecs.append(EXPECTED["multicrop_130x97.std"][n].astype(np.float64))
        slack.append(bound_std + 1e-5)
    for n in d.freq[9:]:
        plane = fr.gray256(img, d.views[n].box)
        raw, bound = fr.raw_features(plane), fr.raw_bound(plane)
        vecs.append(fr.standardize(raw))
        slack.append(fr.std_bound(raw, bound))
    x = torch.tensor(np.stack(vecs), dtype=torch.float64, requires_grad=True)
    want = mlp.double()(x)
    grad, = torch.autograd.grad(want.sum(), x)
    bound = 2 * (grad.abs() * torch.tensor(np.stack(slack))).sum(-1) + 1e-5
    z, z_cells = H.app_freq_logits(torch.from_numpy(img[None]).to(DEV), d, mlp.float().to(DEV))
    assert tuple(z.shape) == (1, 9) and tuple(z_cells.shape) == (16, 1)
    got = torch.cat([z.reshape(-1), z_cells.reshape(-1)]).double().cpu()
    ratio = ((got - want.detach()).abs() / bound).max().item()
    print(f"RATIO app_freq_logits: {ratio:.4f} (largest bound {bound.max().item():.3e})")
    assert ratio <= 1.0
