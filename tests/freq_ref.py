"""Reference restatement of the app's 24-D frequency/SRM feature vector (appv3.py:1618-1728 ``extract_freq_vector`` with
DETECT_USE_CLAHE off) for ``sgl_op_freq_features``, after the conventions at the top of tests/kernel_ref.py: the same
operation in exact integers or float64, and a bound per feature that is computed from this reference alone.

  gray plane   ``gray256``: PIL's ``crop(box).convert("L").resize((256, 256), BICUBIC)`` restated in integers: the luma
               rule, then the two uint8 passes (horizontal, vertical) with 22-bit fixed-point coefficients that are
               made in float64 by add / mul / div only with a sequential sum, as PIL's C doubles are.  Pinned to PIL
               itself byte for byte in tests/test_freq_features_host.py.
  statistics   ``int_stats``: times 255 * abs-sum the SRM responses are integers, times 255 * 2 and 255 * 4 so are the
               two Haar levels; the power sums are taken in int64 (worst case 2040^4 * 65536 = 1.1e18) and the central
               moments in Python integers, so the only error left in a kernel that does the same is the final rounding.
  spectrum     ``spectrum``: float64 FFT of plane / 255 and the app's band / bucket / histogram / sector rules on the
               index tables of ``geometry`` (the app's own torch calls and dtypes).
  bounds       ``raw_bound`` / ``std_bound``, derived below.

The error model.  The kernel transforms in fp64 and rounds every bin to fp32, so a bin's error is
``e_i = 2 * 2^-24 * |F_i| + FFT_C * 16 * 2^-53 * rms|F|``: the rounding of its two components (sqrt(2) units of its
size, rounded up to 2), and the fp64 transform's own error: log2(65536) = 16 radix-2 passes, each a rounded twiddle, two
products and two sums on values of the spectrum's root-mean-square size (Parseval, pass by pass), below 3 units of 2^-53
per pass taken linearly over the passes; FFT_C = 4 is that 3 rounded up to a power of two.  (An fp32 transform would
put FFT_C * 16 * 2^-24 * rms|F| on every bin, four orders above the small bins' own rounding: see csrc/freq_features.hip.)
Propagation is linear (worst case) throughout: a sum of |F| over a set moves by the sum of e_i, a mean of
log(|F| + 1e-6) by the mean of e_i / (|F_i| + 1e-6) (first order), each plus the fp32 rounding of the magnitude, the
logarithm and the running sums; a ratio a / b moves by the quotient rule.  The phase of a bin moves by at most
e_i / |F_i|, and by 4 * 2^-24 * pi for the fp32 atan2 and bin arithmetic.
"""
import math

import numpy as np
import torch

N = 256
U32 = 2.0 ** -24
EPS = 1e-6
FFT_C = 4.0
PRECISION_BITS = 22
SRM = [np.array([[0, 0, 0, 0, 0], [0, -1, 2, -1, 0], [0, 2, -4, 2, 0], [0, -1, 2, -1, 0], [0, 0, 0, 0, 0]], dtype=np.int64),
       np.array([[-1, 2, -1], [2, -4, 2], [-1, 2, -1]], dtype=np.int64),
       np.array([[0, -1, 0], [-1, 4, -1], [0, -1, 0]], dtype=np.int64)]
NAMES = ["El/Et", "Em/Et", "Eh/Et", "Eh/El", "slope", "anis", "entropy",
         "cA1", "cH1", "cV1", "cD1", "cA2", "cH2", "cV2", "cD2",
         "srm0_mean", "srm0_var", "srm0_kurt", "srm1_mean", "srm1_var", "srm1_kurt", "srm2_mean", "srm2_var", "srm2_kurt"]


# ---------------------------------------------------------------------------------------------------------------
# gray plane
# ---------------------------------------------------------------------------------------------------------------
def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def coeffs(in_size, out_size=N):
    """(xmin[out], count[out], k[out, ksize] int64): PIL's precompute_coeffs + normalize_coeffs_8bpc for the window
    [0, in_size).  Entries past ``count`` are zero."""
    scale = float(in_size) / float(out_size)
    fs = scale if scale >= 1.0 else 1.0
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    cnt = xmax - xmin
    j = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic(((j + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(j < cnt[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                    # the sequential sum (np.sum is pairwise)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)   # trunc
    return xmin, cnt, np.where(j < cnt[:, None], k, 0)


def _pass(plane, in_size):
    """One resample pass along the last axis of an int64 plane (rows, in_size) -> (rows, 256), uint8 range."""
    xmin, cnt, k = coeffs(in_size)
    idx = np.minimum(xmin[:, None] + np.arange(k.shape[1])[None, :], in_size - 1)     # padded taps carry k = 0
    acc = np.einsum("roj,oj->ro", plane[:, idx], k) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255)


def luma(rgb):
    rgb = rgb.astype(np.int64)
    return (19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 0x8000) >> 16


def gray256(image_u8, box):
    """(256, 256) uint8 of the window ``box = (x0, y0, x1, y1)`` of an (H, W, 3) uint8 image."""
    x0, y0, x1, y1 = box
    g = luma(np.asarray(image_u8)[y0:y1, x0:x1])
    g = _pass(g, x1 - x0)                                # horizontal: (h, 256)
    g = _pass(np.ascontiguousarray(g.T), y1 - y0).T      # vertical: (256, 256)
    return g.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# exact-integer statistics: 8 wavelet energies, 3 x (mean, variance, kurtosis)
# ---------------------------------------------------------------------------------------------------------------
def haar_level(a):
    """2 x 2 Haar sums of an integer plane, unnormalised: (cA, cH, cV, cD) * 2 of the db1 convention (cH: detail along
    height, cV: along width)."""
    p, q, r, s = a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]
    return p + q + r + s, p + q - r - s, p - q + r - s, p - q - r + s


def srm_response(plane, k):
    """Integer response sum k * p with zero padding k // 2 (cross-correlation, as conv2d; the kernels are symmetric)."""
    r = k.shape[0] // 2
    pad = np.pad(plane.astype(np.int64), r)
    out = np.zeros((N, N), dtype=np.int64)
    for dy in range(k.shape[0]):
        for dx in range(k.shape[1]):
            if k[dy, dx]:
                out += int(k[dy, dx]) * pad[dy:dy + N, dx:dx + N]
    return out


def int_sums(plane):
    """The 20 integer sums the kernel accumulates: 8 x sum c^2 (level 1 times 510, level 2 times 1020), then per SRM
    kernel sum n, n^2, n^3, n^4."""
    p = plane.astype(np.int64)
    l1 = haar_level(p)
    l2 = haar_level(l1[0])
    sums = [int((c * c).sum()) for c in l1 + l2]
    for k in SRM:
        n = srm_response(p, k)
        sums += [int(n.sum()), int((n * n).sum()), int((n ** 3).sum()), int((n ** 4).sum())]
    return sums


def int_stats(plane):
    """The 17 exact-integer features in float64: 8 wavelet, 9 SRM."""
    s = int_sums(plane)
    out = [s[i] / (16384.0 * (255.0 * 2) ** 2) for i in range(4)] + [s[4 + i] / (4096.0 * (255.0 * 4) ** 2) for i in range(4)]
    M = N * N
    for f, k in enumerate(SRM):
        s1, s2, s3, s4 = s[8 + 4 * f:12 + 4 * f]
        scale = 1.0 / (255.0 * (float(np.abs(k).sum()) + EPS))
        c2 = M * s2 - s1 * s1                                                  # M^2 * variance, exact
        c4 = M ** 3 * s4 - 4 * M * M * s1 * s3 + 6 * M * s1 * s1 * s2 - 3 * s1 ** 4   # M^4 * fourth central moment, exact
        mean = scale * (s1 / M)
        var = scale * scale * (c2 / float(M * M))
        m4 = scale ** 4 * (c4 / float(M ** 4))
        out += [mean, var, m4 / (var + EPS) ** 2]
    return out


# ---------------------------------------------------------------------------------------------------------------
# spectrum
# ---------------------------------------------------------------------------------------------------------------
NONE = 255
_geometry = None


def geometry():
    """(band, bucket, sector) uint8 (256, 256) over the fftshift-ed plane, by the app's own torch calls and dtypes;
    255 = belongs to none (bucket: the DC pixel at -1 and anything at 39; sector: the atan2 == pi half-row)."""
    global _geometry
    if _geometry is None:
        h = w = N
        cy, cx = h // 2, w // 2
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        r = torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
        rmax = float(r.max())
        r1, r2 = 0.15 * rmax, 0.45 * rmax
        band = torch.full((h, w), 2, dtype=torch.uint8)
        band[(r > r1) & (r <= r2)] = 1
        band[r <= r1] = 0
        rb = torch.logspace(math.log10(1.0), math.log10(rmax + 1.0), 40)
        ridx = (torch.bucketize(r.flatten() + 1.0, rb) - 1).view(h, w)
        bucket = torch.where((ridx >= 0) & (ridx < 39), ridx, torch.full_like(ridx, NONE)).to(torch.uint8)
        ang = torch.atan2(yy - cy, xx - cx)
        sector = torch.full((h, w), NONE, dtype=torch.uint8)
        for n, a0 in enumerate(np.linspace(-math.pi, math.pi, 8, endpoint=False)):
            sector[(ang >= a0) & (ang < a0 + math.pi / 4)] = n
        _geometry = (band, bucket, sector)
    return _geometry


def _entropy(hist):
    """The app's own fp32 formula on the integer counts: its 1e-6 terms sit at the fp32 rounding of the probabilities, so
    the formula is part of the definition (an all-in-one-bin histogram gives -log(1 + 1e-6 in fp32), not -1e-6)."""
    h = torch.from_numpy(hist).float()
    p = h / (h.sum() + EPS)
    return float(-(p * torch.log(p + EPS)).sum().item())


def spectrum(plane):
    """The 7 spectral features in float64 and what the bounds need."""
    band, bucket, sector = (t.numpy() for t in geometry())
    F = np.fft.fftshift(np.fft.fft2(plane.astype(np.float64) / 255.0))
    mag, phase = np.abs(F), np.angle(F)
    E = [float(mag[band == b].sum()) for b in range(3)]
    Et = float(mag.sum()) + EPS
    lg = np.log(mag + 1e-6)
    cnt = np.array([(bucket == b).sum() for b in range(39)])
    mu = np.array([lg[bucket == b].mean() if cnt[b] else 0.0 for b in range(39)])
    xs = np.arange(39.0)
    wslope = (xs - xs.mean()) / ((xs - xs.mean()) ** 2).sum()
    slope = float((wslope * mu).sum())
    pos = np.minimum(np.floor((phase + math.pi) * 50 / (2 * math.pi)).astype(np.int64), 49)
    hist = np.bincount(pos.ravel(), minlength=50).astype(np.float64)
    sect = np.array([mag[sector == s].mean() for s in range(8)])
    feats = [E[0] / Et, E[1] / Et, E[2] / Et, (E[2] + EPS) / (E[0] + EPS), slope, float(np.var(sect)), _entropy(hist)]
    aux = dict(mag=mag, phase=phase, E=E, Et=Et, lg=lg, cnt=cnt, mu=mu, wslope=wslope, hist=hist, sect=sect,
               band=band, bucket=bucket, sector=sector)
    return feats, aux


def raw_features(plane):
    """(24,) float64 of a (256, 256) uint8 gray plane, in the app's order: 7 spectral, 8 wavelet, 9 SRM."""
    f, _ = spectrum(plane)
    return np.array(f + int_stats(plane), dtype=np.float64)


def standardize(v):
    v = np.asarray(v, dtype=np.float64)
    s = v.std(ddof=1)
    return np.zeros_like(v) if s < 1e-6 else (v - v.mean()) / (s + 1e-6)


# ---------------------------------------------------------------------------------------------------------------
# bounds (from the float64 reference alone)
# ---------------------------------------------------------------------------------------------------------------
def raw_bound(plane, transform="fp64"):
    """(24,) per-feature bound on |kernel - float64 reference|; see the module docstring.  ``transform="fp32"`` is the
    same propagation for an fp32 FFT (every bin carries 16 * 2^-24 * rms|F|, one unit per pass): not what the kernel
    does, kept so that the reason it does not can be recomputed (tests/test_freq_features_host.py)."""
    f, a = spectrum(plane)
    M = N * N
    mag = a["mag"]
    rms = math.sqrt(float((mag ** 2).mean()))
    e = 2 * U32 * mag + FFT_C * 16 * 2.0 ** -53 * rms                       # per bin
    if transform == "fp32":
        e = np.full_like(mag, 16 * U32 * rms)
    # band sums: e_i per member plus the fp32 rounding of |F| (2 units: the squares, their sum, the root) and of a sum
    # whose partial sums form a tree of depth <= 16
    dE = [float(e[a["band"] == b].sum()) + (2 + 16) * U32 * a["E"][b] for b in range(3)]
    dEt = sum(dE)
    Et = a["Et"]
    b = [dE[i] / Et + a["E"][i] * dEt / Et ** 2 for i in range(3)]
    El, Eh = a["E"][0] + EPS, a["E"][2] + EPS
    b.append(dE[2] / El + Eh * dE[0] / El ** 2)
    # log means: e_i / (|F_i| + 1e-6) per member, the logarithm's own rounding (2 units of |log|, 2 of 1) and the mean's
    dlg = e / (mag + 1e-6) + U32 * (2 * np.abs(a["lg"]) + 2)
    dmu = np.array([dlg[a["bucket"] == k].mean() + 16 * U32 * np.abs(a["lg"][a["bucket"] == k]).mean() if a["cnt"][k] else 0.0
                    for k in range(39)])
    b.append(float((np.abs(a["wslope"]) * dmu).sum()))
    # anisotropy: variance of 8 means, each moving by its members' mean e_i plus summation rounding
    ds = np.array([e[a["sector"] == k].mean() for k in range(8)]) + (2 + 16) * U32 * a["sect"]
    dev = np.abs(a["sect"] - a["sect"].mean())
    b.append(float((2 * dev * (ds + ds.mean())).sum() / 8 + ((ds + ds.mean()) ** 2).sum() / 8))
    # entropy: samples whose float64 phase lies within the phase error of a histogram edge may change bin; one moved
    # sample changes -sum p log(p + eps) by at most (1 / M) * the spread of d/dp over the histogram
    if rms == 0.0:
        moved = 0                                        # an all-zero spectrum is exact: every phase is +0, one bin
    else:
        dphi = e / np.maximum(mag, 1e-300) + 4 * U32 * math.pi
        t = (a["phase"] + math.pi) * 50 / (2 * math.pi)
        dist = np.abs(t - np.round(t)) * (2 * math.pi / 50)
        moved = int((dist <= dphi).sum())
    p = a["hist"] / (a["hist"].sum() + EPS)
    pm = np.clip(np.stack([p - moved / M, p + moved / M]), 0.0, 1.0)
    g = np.log(pm + EPS) + pm / (pm + EPS)
    b.append(moved / M * float(g.max() - g.min()) + 64 * U32)         # 50 fp32 terms of size <= 0.37, summed
    # exact-integer features: the final fp32 rounding only
    exact = np.abs(np.array(int_stats(plane))) * (U32 + 2.0 ** -48)      # and the double arithmetic before it
    return np.concatenate([np.array(b) + np.abs(np.array(f)) * U32, exact])


def std_bound(raw, bound):
    """(24,) bound on the standardised vector given the raw features and their bounds: the mean moves by at most
    mean(bound), the unbiased std (1-Lipschitz in the centred vector / sqrt(n - 1)) by |bound|_2 / sqrt(n - 1), and the
    result is rounded to fp32."""
    raw, bound = np.asarray(raw, np.float64), np.asarray(bound, np.float64)
    s = raw.std(ddof=1)
    if s < 1e-6:
        return np.zeros_like(raw)
    ds = float(np.sqrt((bound ** 2).sum() / (raw.size - 1)))
    z = (raw - raw.mean()) / (s + 1e-6)
    return (bound + bound.mean()) / (s + 1e-6) + np.abs(z) * ds / (s + 1e-6 - ds) + np.abs(z) * U32
