// GPU input pipeline, first slice of SURVEY.md §8f row 2: the reference's per-batch GPU transform
//     K.Resize(target_resolution, antialias=True) -> K.Normalize(mean=0.5, std=0.5)      cifake_binary_classifier.py:1791-1794
//     (+ optionally MixUp: lam * images + (1 - lam) * images[index]                       cifake_binary_classifier.py:812-817)
// fused with the patch gather of the patch-embedding convolution (TF:modeling_siglip.py:175-185): source images
// (decoded uint8 NHWC bytes, or the float [0,1] NCHW tensors the reference's CPU transform produces) are resampled,
// normalised and written straight into the bf16 patch-major A operand [B*gh*gw][Kp] of the patch GEMM — the fp32
// (B,3,S,S) pixel tensor of the reference is never materialised and the im2col pass (encoder.hip) disappears.
//
// Resampling = separable triangle filter with the support stretched by the down-scale factor: the arithmetic of
// torch's upsample_bilinear2d(antialias=True) (aten/native/cpu/UpSampleKernel.cpp, _compute_indices_weights_aa), which
// is what torchvision Resize(antialias=True) runs in the reference's CPU transform (cifake...:1795-1797).  kornia (the
// GPU transform) is not installed here: its result is "parity unpinned" (it blurs with a Gaussian before sampling).
// HBM-bound; one thread = one operand element (coalesced bf16 stores along k), source taps come from L1/L2.
//
// Map: aa_axis / aa_w / resample_px   the one filter of every kernel      | OutLayout   where an output element goes
//      preprocess_kernel, aug_* + preprocess_aug_kernel, preprocess_views_kernel   the three forward transforms
//      AxisTables + views_bwd_tables_kernel + bwd_filter_sum<NC>          the tables and the sum of both adjoints
//      preprocess_bwd_kernel, preprocess_views_bwd_kernel                 the adjoints (float source, NCHW output)
//      aug_hue_bwd, aug_colour_bwd, aug_bwd_*_kernel                      the adjoint of the augmenting transform
//      check_args, views_check, dispatch_src_out, extern "C"              refusals, type dispatch, the entry points
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.hip.h"
#include "kernels.h"
#include "siglip_hip.h"

namespace sgl {

struct AaAxis {
  int lo, n;
  float center, invscale, inv_total;
};

// taps of output index i along one axis (in -> out), weights w_j = tri((j + lo - center + 0.5) * invscale) / total
__device__ __forceinline__ AaAxis aa_axis(int i, int in, float scale) {
  AaAxis a;
  const float support = scale >= 1.0f ? scale : 1.0f;
  a.invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
  a.center = scale * ((float)i + 0.5f);
  int lo = (int)(a.center - support + 0.5f);
  if (lo < 0) lo = 0;
  int hi = (int)(a.center + support + 0.5f);
  if (hi > in) hi = in;
  a.lo = lo;
  a.n = hi - lo;
  float total = 0.f;
  for (int j = 0; j < a.n; ++j) {
    float x = ((float)(j + lo) - a.center + 0.5f) * a.invscale;
    x = x < 0.f ? -x : x;
    total += x < 1.0f ? 1.0f - x : 0.f;
  }
  a.inv_total = total != 0.f ? 1.0f / total : 0.f;
  return a;
}
__device__ __forceinline__ float aa_w(const AaAxis& a, int j) {
  float x = ((float)(j + a.lo) - a.center + 0.5f) * a.invscale;
  x = x < 0.f ? -x : x;
  return (x < 1.0f ? 1.0f - x : 0.f) * a.inv_total;
}

template <bool SRC_U8>
__device__ __forceinline__ float src_px(const void* src, int b, int c, int y, int x, int Hs, int Ws) {
  if constexpr (SRC_U8)   // NHWC bytes
    return (float)reinterpret_cast<const uint8_t*>(src)[(((size_t)b * Hs + y) * Ws + x) * 3 + c] * (1.0f / 255.0f);
  else                    // NCHW float in [0, 1]
    return reinterpret_cast<const float*>(src)[(((size_t)b * 3 + c) * Hs + y) * Ws + x];
}

// output pixel (oy, ox) of the h x w image px(y, x) resized by (sy, sx): the one filter loop of every forward kernel here
template <typename Px>
__device__ __forceinline__ float resample_px(Px px, int oy, int ox, int h, int w, float sy, float sx) {
  if (sy == 1.0f && sx == 1.0f) return px(oy, ox);
  const AaAxis ay = aa_axis(oy, h, sy), ax = aa_axis(ox, w, sx);
  float acc = 0.f;
  for (int jy = 0; jy < ay.n; ++jy) {
    float row = 0.f;
    for (int jx = 0; jx < ax.n; ++jx) row += aa_w(ax, jx) * px(ay.lo + jy, ax.lo + jx);
    acc += aa_w(ay, jy) * row;
  }
  return acc;
}

template <bool SRC_U8>
__device__ __forceinline__ float resample(const void* src, int b, int c, int oy, int ox, int Hs, int Ws, float sy,
                                          float sx) {
  return resample_px([&](int y, int x) { return src_px<SRC_U8>(src, b, c, y, x, Hs, Ws); }, oy, ox, Hs, Ws, sy, sx);
}

// The two output layouts of the forward transforms, n = the image or view:
// patch_major: out[(n*g + gy)*g + gx][k], k = c*P*P + ky*P + kx (k >= 3*P*P zero), g = S / P | else out[n][c][y][x]
struct OutPx {
  int n, c, oy, ox;
  bool live;                                             // false: a K padding column, stored as zero
};
struct OutLayout {
  int S, P, Kp, g, patch_major;                          // g = patch_major ? S / P : 0

  __host__ __device__ size_t elems(int n) const { return patch_major ? (size_t)n * g * g * Kp : (size_t)n * 3 * S * S; }
  __device__ __forceinline__ OutPx decode(size_t idx) const {
    OutPx o;
    o.live = true;
    if (patch_major) {
      const int k = (int)(idx % Kp);
      const size_t m = idx / Kp;
      const int gx = (int)(m % g), gy = (int)((m / g) % g);
      o.n = (int)(m / ((size_t)g * g));
      o.live = k < 3 * P * P;
      o.c = k / (P * P);
      const int r = k - o.c * P * P;
      o.oy = gy * P + r / P;
      o.ox = gx * P + r % P;
    } else {
      o.ox = (int)(idx % S);
      o.oy = (int)((idx / S) % S);
      o.c = (int)((idx / ((size_t)S * S)) % 3);
      o.n = (int)(idx / ((size_t)3 * S * S));
    }
    return o;
  }
  __device__ __forceinline__ size_t offset(int n, int c, int oy, int ox) const {   // the inverse of decode
    if (patch_major) return (((size_t)n * g + oy / P) * g + ox / P) * Kp + (size_t)c * P * P + (oy % P) * P + (ox % P);
    return (((size_t)n * 3 + c) * S + oy) * S + ox;
  }
};

template <bool SRC_U8, typename TOut>
__global__ __launch_bounds__(256) void preprocess_kernel(const void* __restrict__ src, TOut* __restrict__ out, int B,
                                                         int Hs, int Ws, const OutLayout L, float mean, float inv_std,
                                                         const int* __restrict__ mix_index, float lam) {
  const size_t total = L.elems(B);
  const float sy = (float)Hs / (float)L.S, sx = (float)Ws / (float)L.S;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const OutPx o = L.decode(idx);
    float v = 0.f;
    if (o.live) {
      v = resample<SRC_U8>(src, o.n, o.c, o.oy, o.ox, Hs, Ws, sy, sx);
      if (mix_index)
        v = lam * v + (1.0f - lam) * resample<SRC_U8>(src, mix_index[o.n], o.c, o.oy, o.ox, Hs, Ws, sy, sx);
      v = (v - mean) * inv_std;
    }
    Elem<TOut>::st(out + idx, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Augmentation branch of the video trainer's GPU transform (hidf_video_classifier.py:2868-2874), fused into the same pass:
//     K.Resize(S, antialias=True) -> K.RandomHorizontalFlip(p=0.5) -> K.RandomRotation(degrees=5, p=0.3)
//     -> K.ColorJitter(brightness=0.1, contrast=0.1, saturation=0.1, hue=0.05, p=0.3) -> K.Normalize(0.5, 0.5)
// Randomness stays with the caller: per-sample parameters arrive in a device table (sgl_aug_sample).  Definitions used
// (kornia is not installed: "parity unpinned" against it; oracle/preprocess_oracle.py restates exactly these):
//   flip      out(y, x) = in(y, S-1-x)
//   rotation  about the image centre ((S-1)/2, (S-1)/2), positive angle counter-clockwise (OpenCV / kornia
//             get_rotation_matrix2d), out(p) = in(M^-1 p) sampled bilinearly, zeros outside
//   colour    torchvision-style operators on [0,1] RGB, each clamped to [0,1], applied in the order given per sample:
//             0 brightness x*f | 1 contrast (x - m)*f + m, m = mean of the image's grey level at that point of the chain |
//             2 saturation (x - grey)*f + grey | 3 hue: RGB -> HSV, h = frac(h + shift), HSV -> RGB; grey = .299R+.587G+.114B
// The contrast operator needs a per-image mean of the partly transformed image: a first launch (aug_mean_kernel, one
// workgroup per image, fixed summation order) evaluates the chain up to the contrast step and reduces it.
struct AugSample {   // == sgl_aug_sample
  float flip, cos_a, sin_a, brightness, contrast, saturation, hue;
  int order[4];
  int reserved;
};

__device__ __forceinline__ float aug_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }
__device__ __forceinline__ float aug_grey(const float* c) { return 0.299f * c[0] + 0.587f * c[1] + 0.114f * c[2]; }

__device__ __forceinline__ void aug_hue(float* c, float shift) {
  const float r = c[0], g = c[1], b = c[2];
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float sat = cr / (eq ? 1.0f : maxc);
  const float crd = eq ? 1.0f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  const float hr = (maxc == r) ? (bc - gc) : 0.f;
  const float hg = (maxc == g && maxc != r) ? (2.0f + rc - bc) : 0.f;
  const float hb = (maxc != g && maxc != r) ? (4.0f + gc - rc) : 0.f;
  float h = (hr + hg + hb) / 6.0f + 1.0f;
  h = h - floorf(h);                 // fmod(., 1)
  h = h + shift;
  h = h - floorf(h);                 // (h + shift) % 1
  const float v = maxc;
  const float h6 = h * 6.0f;
  const float fi = floorf(h6);
  const float f = h6 - fi;
  int i = (int)fi % 6;
  const float p = aug_clamp01(v * (1.0f - sat));
  const float q = aug_clamp01(v * (1.0f - f * sat));
  const float t = aug_clamp01(v * (1.0f - (1.0f - f) * sat));
  switch (i) {
    case 0: c[0] = v; c[1] = t; c[2] = p; break;
    case 1: c[0] = q; c[1] = v; c[2] = p; break;
    case 2: c[0] = p; c[1] = v; c[2] = t; break;
    case 3: c[0] = p; c[1] = q; c[2] = v; break;
    case 4: c[0] = t; c[1] = p; c[2] = v; break;
    default: c[0] = v; c[1] = p; c[2] = q; break;
  }
}

// resized + flipped + rotated RGB of output pixel (oy, ox)
template <bool SRC_U8>
__device__ __forceinline__ void aug_geo(const void* src, int b, int oy, int ox, int Hs, int Ws, int S, float sy, float sx,
                                        const AugSample& a, float* rgb) {
  const bool flip = a.flip != 0.f;
  auto px = [&](int c, int y, int x) {
    return resample<SRC_U8>(src, b, c, y, flip ? S - 1 - x : x, Hs, Ws, sy, sx);
  };
  if (a.sin_a == 0.f && a.cos_a == 1.f) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = px(c, oy, ox);
    return;
  }
  const float ctr = 0.5f * (float)(S - 1);
  const float dx = (float)ox - ctr, dy = (float)oy - ctr;
  const float xs = a.cos_a * dx - a.sin_a * dy + ctr;
  const float ys = a.sin_a * dx + a.cos_a * dy + ctr;
  const float x0f = floorf(xs), y0f = floorf(ys);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float fx = xs - x0f, fy = ys - y0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = 0.f;
#pragma unroll
    for (int jy = 0; jy < 2; ++jy)
#pragma unroll
      for (int jx = 0; jx < 2; ++jx) {
        const int yy = y0 + jy, xx = x0 + jx;
        const float w = (jy ? fy : 1.0f - fy) * (jx ? fx : 1.0f - fx);
        if (yy >= 0 && yy < S && xx >= 0 && xx < S && w != 0.f) v += w * px(c, yy, xx);
      }
    rgb[c] = v;
  }
}

// one operator of the colour chain on rgb, in place: the one place its arithmetic is written (the adjoint recomputes with it)
__device__ __forceinline__ void aug_colour_op(float* rgb, const AugSample& a, int op, float grey_mean) {
  if (op == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = aug_clamp01(rgb[c] * a.brightness);
  } else if (op == 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = aug_clamp01((rgb[c] - grey_mean) * a.contrast + grey_mean);
  } else if (op == 2) {
    const float g = aug_grey(rgb);
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = aug_clamp01((rgb[c] - g) * a.saturation + g);
  } else {
    aug_hue(rgb, a.hue);
  }
}

// colour chain on rgb; stop_before_contrast: evaluate only the operators in front of the contrast step (mean pre-pass)
__device__ __forceinline__ void aug_colour(float* rgb, const AugSample& a, float grey_mean, bool stop_before_contrast) {
  if (a.order[0] < 0) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = a.order[k];
    if (op == 1 && stop_before_contrast) return;
    aug_colour_op(rgb, a, op, grey_mean);
  }
}

template <bool SRC_U8>
__global__ __launch_bounds__(256) void aug_mean_kernel(const void* __restrict__ src, int Hs, int Ws, int S,
                                                       const AugSample* __restrict__ aug, float* __restrict__ grey_mean) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const AugSample a = aug[b];
  bool need = false;
  if (a.order[0] >= 0)
    for (int k = 0; k < 4; ++k) need = need || a.order[k] == 1;
  if (!need) {
    if (threadIdx.x == 0) grey_mean[b] = 0.f;
    return;
  }
  const float sy = (float)Hs / (float)S, sx = (float)Ws / (float)S;
  float acc = 0.f;
  for (int i = threadIdx.x; i < S * S; i += 256) {
    float rgb[3];
    aug_geo<SRC_U8>(src, b, i / S, i % S, Hs, Ws, S, sy, sx, a, rgb);
    aug_colour(rgb, a, 0.f, true);
    acc += aug_grey(rgb);
  }
  acc = wave_sum(acc);
  if (lane_id() == 0) red[wave_id()] = acc;
  __syncthreads();
  if (threadIdx.x == 0) grey_mean[b] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)(S * S);
}

template <bool SRC_U8, typename TOut>
__global__ __launch_bounds__(256) void preprocess_aug_kernel(const void* __restrict__ src, TOut* __restrict__ out, int B,
                                                             int Hs, int Ws, const OutLayout L, float mean,
                                                             float inv_std, const AugSample* __restrict__ aug,
                                                             const float* __restrict__ grey_mean) {
  // one thread = one output PIXEL (all three channels: the colour operators mix them)
  const int S = L.S;
  const int side = L.patch_major ? L.g * L.P : S;       // pixels past the last whole patch are dropped ('valid' conv)
  const size_t total = (size_t)B * side * side;
  const float sy = (float)Hs / (float)S, sx = (float)Ws / (float)S;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int ox = (int)(idx % side), oy = (int)((idx / side) % side), b = (int)(idx / ((size_t)side * side));
    const AugSample a = aug[b];
    float rgb[3];
    aug_geo<SRC_U8>(src, b, oy, ox, Hs, Ws, S, sy, sx, a, rgb);
    aug_colour(rgb, a, grey_mean[b], false);
#pragma unroll
    for (int c = 0; c < 3; ++c) Elem<TOut>::st(out + L.offset(b, c, oy, ox), (rgb[c] - mean) * inv_std);
  }
}

// zero the K padding columns [3*P*P, Kp) of a patch-major operand (the augmentation kernel writes pixels only)
template <typename TOut>
__global__ __launch_bounds__(256) void patch_pad_zero_kernel(TOut* __restrict__ out, size_t rows, int K0, int Kp) {
  const int padw = Kp - K0;
  const size_t total = rows * (size_t)padw;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256)
    Elem<TOut>::st(out + (idx / padw) * Kp + K0 + idx % padw, 0.f);
}

// ---------------------------------------------------------------------------------------------------------------
// Test-time views of the app (appv3.py:3214-3250 detect_core, :3315 make_multicrops, :3381 compute_patch_grid): V windows
// onto B same-size sources in one pass.  A view = integer crop box -> quarter turns (exact, or on PIL's fixed canvas:
// Image.rotate(90 k) with expand=False, nearest, fill 0) -> mirror -> the resize + normalise of preprocess_kernel with
// `in` = the oriented extents.  The oriented image is never built: a tap (y, x) of it is mapped to a crop coordinate by
// an integer affine map and read from the source (or is zero outside the canvas); include/siglip_hip.h has the rules.
// The records travel by value in the kernel arguments (64 x 32 bytes of the 4 KB a launch may carry): no device table,
// no copy, nothing to keep alive, graph-capturable.  Same thread mapping and store pattern as preprocess_kernel.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kViewChunk = 64;
struct ViewChunk {
  sgl_view v[kViewChunk];
};

// oriented extents of a record: an exact odd turn swaps them, a turn on the kept canvas does not
__host__ __device__ __forceinline__ void view_extent(const sgl_view& r, int* oh, int* ow) {
  const int w = r.x1 - r.x0, h = r.y1 - r.y0;
  const bool swap = (r.turns & 1) && !r.keep_canvas;
  *oh = swap ? w : h;
  *ow = swap ? h : w;
}

// crop coordinate of oriented pixel (y, x): cx = ax + axx x + axy y, cy = ay + ayx x + ayy y; outside [0,w) x [0,h): zero
struct ViewMap {
  int src, x0, y0, w, h, oh, ow;
  int ax, axx, axy, ay, ayx, ayy;
};

__device__ __forceinline__ ViewMap view_map(const sgl_view& r) {
  ViewMap m;
  m.src = r.src, m.x0 = r.x0, m.y0 = r.y0;
  const int w = m.w = r.x1 - r.x0, h = m.h = r.y1 - r.y0;
  view_extent(r, &m.oh, &m.ow);
  m.ax = 0, m.axx = 1, m.axy = 0, m.ay = 0, m.ayx = 0, m.ayy = 1;
  if (r.turns == 2) {                                    // exact on either canvas (PIL: transpose(ROTATE_180))
    m.ax = w - 1, m.axx = -1, m.ay = h - 1, m.ayy = -1;
  } else if (r.turns != 0) {
    // exact: rot90(C, 1)[y][x] = C[x][w-1-y], rot90(C, 3)[y][x] = C[h-1-x][y].  Kept canvas: PIL's nearest affine
    // transform samples floor((w+h)/2 - (y + 0.5)), floor((h-w)/2 + (x + 0.5)) at one turn (mirrored roles at three);
    // >> 1 is the floor for the negative half-integers too.  w == h makes the two rules coincide.
    const int hi = r.keep_canvas ? (w + h - 1) >> 1 : (r.turns == 1 ? w - 1 : h - 1);
    const int lo = r.keep_canvas ? ((r.turns == 1 ? h - w : w - h) + 1) >> 1 : 0;
    m.axx = 0, m.ayy = 0;
    if (r.turns == 1) m.ax = hi, m.axy = -1, m.ay = lo, m.ayx = 1;
    else m.ax = lo, m.axy = 1, m.ay = hi, m.ayx = -1;
  }
  if (r.flip) {                                          // x -> ow - 1 - x
    m.ax += m.axx * (m.ow - 1), m.axx = -m.axx;
    m.ay += m.ayx * (m.ow - 1), m.ayx = -m.ayx;
  }
  return m;
}

template <bool SRC_U8>
__device__ __forceinline__ float view_px(const void* src, const ViewMap& m, int c, int y, int x, int Hs, int Ws) {
  const int cx = m.ax + m.axx * x + m.axy * y, cy = m.ay + m.ayx * x + m.ayy * y;
  if (cx < 0 || cx >= m.w || cy < 0 || cy >= m.h) return 0.f;
  return src_px<SRC_U8>(src, m.src, c, m.y0 + cy, m.x0 + cx, Hs, Ws);
}

// out: the rows of this chunk's first view onward; layouts as preprocess_kernel with b = the view's index in the chunk
template <bool SRC_U8, typename TOut>
__global__ __launch_bounds__(256) void preprocess_views_kernel(const void* __restrict__ src, TOut* __restrict__ out,
                                                               const ViewChunk chunk, int nv, int Hs, int Ws,
                                                               const OutLayout L, float mean, float inv_std) {
  const size_t total = L.elems(nv);
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const OutPx o = L.decode(idx);
    float val = 0.f;
    if (o.live) {
      const ViewMap m = view_map(chunk.v[o.n]);
      const float sy = (float)m.oh / (float)L.S, sx = (float)m.ow / (float)L.S;
      val = resample_px([&](int y, int x) { return view_px<SRC_U8>(src, m, o.c, y, x, Hs, Ws); }, o.oy, o.ox, m.oh, m.ow,
                        sy, sx);
      val = (val - mean) * inv_std;
    }
    Elem<TOut>::st(out + idx, val);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Adjoint of preprocess_kernel<false, float>(patch_major = 0) with respect to a float source: the forward is linear,
//     out[b] = (lam Wy src[b] Wx^T + (1 - lam) Wy src[mix[b]] Wx^T - mean) / std,
// so d_src[b] = Wy^T (lam G[b] + (1 - lam) sum_{j : mix[j] == b} G[j]) Wx / std with the SAME fp32 weights (aa_axis / aa_w).
// Gather form: one thread = one source element, which sums the outputs whose taps include it; nothing is scattered, no
// atomics, every element of d_src is stored exactly once, and the order of the sums is fixed (j, then oy, then ox).
// A pre-pass (views_bwd_tables_kernel, for the one full-frame record) writes two small tables per axis into caller
// scratch, so that the per-element loop neither normalises a filter (up to 33 taps per output at ratio 16) nor searches:
//   AaAxis  [S]   the forward's filter of every output index
//   SrcSpan [in]  the outputs [first, first + count) whose taps [lo, hi) include source index j.  lo and hi are
//                 non-decreasing in the output index, so the set is one range; it is found by testing lo <= j < hi with
//                 the forward's own fp32 expressions (aa_axis) over a window that is wider than any rounding of the
//                 inverted formula could move it: inverting in floating point alone would drop or invent a boundary tap.
// ---------------------------------------------------------------------------------------------------------------
struct SrcSpan {
  int first, count;
};

__device__ __forceinline__ bool aa_covers(int o, int j, int in, float scale) {
  const AaAxis a = aa_axis(o, in, scale);                // only lo and n are used: the normalisation loop is dead code
  return a.lo <= j && j < a.lo + a.n;
}

__device__ __forceinline__ SrcSpan src_span(int j, int in, int out, float scale) {
  const float support = scale >= 1.0f ? scale : 1.0f;
  // covering outputs satisfy (j + 0.5 - support) / scale - 0.5 <= o < (j + 0.5 + support) / scale - 0.5 in exact arithmetic
  int o0 = (int)floorf(((float)j - support - 1.0f) / scale - 0.5f) - 1;
  int o1 = (int)ceilf(((float)j + support + 1.0f) / scale - 0.5f) + 1;
  if (o0 < 0) o0 = 0;
  if (o1 > out - 1) o1 = out - 1;
  int first = o0;
  while (first <= o1 && !aa_covers(first, j, in, scale)) ++first;
  int end = first;
  while (end <= o1 && aa_covers(end, j, in, scale)) ++end;
  SrcSpan s;
  s.first = first;
  s.count = end - first;
  return s;
}

// One table set, for an oriented image of oh x ow resized to S x S: AaAxis[S] (y), AaAxis[S] (x), SrcSpan[oh], SrcSpan[ow]
struct AxisTables {
  AaAxis *ty, *tx;
  SrcSpan *ry, *rx;
};

__host__ __device__ __forceinline__ size_t view_table_bytes(int oh, int ow, int S) {
  if (oh == S && ow == S) return 0;                      // the copy shortcut reads no table
  return (size_t)2 * S * sizeof(AaAxis) + ((size_t)oh + (size_t)ow) * sizeof(SrcSpan);
}

__host__ __device__ __forceinline__ AxisTables axis_tables(char* base, int oh, int S) {
  AxisTables t;
  t.ty = reinterpret_cast<AaAxis*>(base);
  t.tx = t.ty + S;
  t.ry = reinterpret_cast<SrcSpan*>(t.tx + S);
  t.rx = t.ry + oh;
  return t;
}

// sum over the outputs of one image that read source element (y, x), for NC channels (planes `plane` apart) side by
// side: out[c] = (Wy^T G[c] Wx)[y, x].  Each weight is evaluated once per tap, then the row sums, then acc: the same
// operations in the same order for every NC, and NC independent loads in flight per tap
template <int NC>
__device__ __forceinline__ void bwd_filter_sum(const float* __restrict__ g, size_t plane, const AxisTables& t, SrcSpan py,
                                               SrcSpan px, int y, int x, int S, float* out) {
  float acc[NC] = {};
  for (int oy = py.first; oy < py.first + py.count; ++oy) {
    const AaAxis ay = t.ty[oy];
    const float* grow = g + (size_t)oy * S;
    float row[NC] = {};
    for (int ox = px.first; ox < px.first + px.count; ++ox) {
      const AaAxis ax = t.tx[ox];
      const float w = aa_w(ax, x - ax.lo);
#pragma unroll
      for (int c = 0; c < NC; ++c) row[c] += w * grow[c * plane + ox];
    }
    const float wy = aa_w(ay, y - ay.lo);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] += wy * row[c];
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) out[c] = acc[c];
}

// t: the tables of the full frame; t.ty == nullptr when Hs == S && Ws == S (the forward's copy shortcut)
__global__ __launch_bounds__(256) void preprocess_bwd_kernel(const float* __restrict__ d_out, float* __restrict__ d_src,
                                                             int B, int Hs, int Ws, int S, float inv_std,
                                                             const int* __restrict__ mix_index, float lam,
                                                             const AxisTables t) {
  const size_t total = (size_t)B * 3 * Hs * Ws;
  const bool copy = t.ty == nullptr;
  const size_t plane = (size_t)S * S;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int x = (int)(idx % Ws), y = (int)((idx / Ws) % Hs);
    const int c = (int)((idx / ((size_t)Hs * Ws)) % 3), b = (int)(idx / ((size_t)3 * Hs * Ws));
    SrcSpan py = {0, 0}, px = {0, 0};
    if (!copy) {
      py = t.ry[y];
      px = t.rx[x];
    }
    auto image = [&](int j) {
      const float* g = d_out + ((size_t)j * 3 + c) * plane;
      float f;
      if (copy) f = g[(size_t)y * S + x];
      else bwd_filter_sum<1>(g, plane, t, py, px, y, x, S, &f);
      return f;
    };
    float v = image(b);
    if (mix_index) {
      v = lam * v;
      const float oml = 1.0f - lam;
      for (int j = 0; j < B; ++j)                        // mix_index need not be a permutation: 0, 1 or many j per b
        if (mix_index[j] == b) v += oml * image(j);
    }
    d_src[idx] = v * inv_std;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Adjoint of preprocess_views_kernel<false, float>(patch_major = 0) with respect to a float source.  Every view is linear
// in the source, out[v] = (Wy_v O_v Wx_v^T - mean) / std with O_v the oriented crop, so
//     d_src[b] = (sum over {v : view v names image b} of orient_v^T (Wy_v^T G[v] Wx_v)) / std.
// The same gather as preprocess_bwd_kernel: every source element (b, c, y, x) has one owner that sums its terms and stores
// it once.  A thread owns the three channels of one source pixel (b, y, x): the map, the spans and the filter weights are
// the same for the three, so they are evaluated once and three independent loads are in flight per tap (the loop is
// bound by load latency, not bandwidth).  A block owns a 16 x 16 pixel tile, a wave four rows of 16: a wave's stores are
// four 64-byte runs, and its reads of G are a few runs whether the view is turned or not (with a whole source row per
// wave a view with an odd turn reads G with stride S, 64 lines per load).  The record loop is wave-uniform and the
// records are kernel arguments.  For every record of its image whose box holds (x, y) the thread
// inverts view_map (a signed permutation plus offset) to the oriented pixel (Y, X), drops the term when that falls off
// the kept canvas, and adds bwd_filter_sum<3> over the two SrcSpans of (Y, X); a view with
// oh == ow == S reads G[v][c][Y][X] (the forward's copy shortcut).  Order per element: view ascending, then oy, then ox;
// one multiply by 1 / std at the end.
// V > 64: one launch per 64 records on the caller's stream; the first stores the partial sum, each later one loads it,
// goes on adding in the same order and stores it back, the last one scales: the bits of one long loop over all V.
// Tables: per view that is not a copy, one AxisTables set in caller scratch at the byte offset that travels next to the
// record; one pre-pass launch per 64 records writes them (aa_axis / src_span).
// ---------------------------------------------------------------------------------------------------------------
struct ViewTableChunk {
  size_t off[kViewChunk];
};

// grid: (blocks over the 2 S + oh + ow entries, views of the chunk)
__global__ __launch_bounds__(256) void views_bwd_tables_kernel(char* __restrict__ scratch, const ViewChunk chunk,
                                                               const ViewTableChunk tabs, int S) {
  const int v = blockIdx.y;
  int oh, ow;
  view_extent(chunk.v[v], &oh, &ow);
  if (oh == S && ow == S) return;
  const AxisTables t = axis_tables(scratch + tabs.off[v], oh, S);
  const float sy = (float)oh / (float)S, sx = (float)ow / (float)S;   // the forward's scales
  const int total = 2 * S + oh + ow;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    if (i < S) t.ty[i] = aa_axis(i, oh, sy);
    else if (i < 2 * S) t.tx[i - S] = aa_axis(i - S, ow, sx);
    else if (i < 2 * S + oh) t.ry[i - 2 * S] = src_span(i - 2 * S, oh, S, sy);
    else t.rx[i - 2 * S - oh] = src_span(i - 2 * S - oh, ow, S, sx);
  }
}

constexpr int kBwdTile = 16;   // 16 x 16 pixels per block: kBwdTile * kBwdTile == the block's 256 threads

// d_out: the rows of this chunk's first view onward.  first: store (no load); last: scale by inv_std.  scratch is read only
__global__ __launch_bounds__(256) void preprocess_views_bwd_kernel(const float* __restrict__ d_out,
                                                                   float* __restrict__ d_src,
                                                                   char* __restrict__ scratch,
                                                                   const ViewChunk chunk, const ViewTableChunk tabs,
                                                                   int nv, int B, int Hs, int Ws, int S, int first,
                                                                   int last, float inv_std) {
  const size_t src_plane = (size_t)Hs * Ws, plane = (size_t)S * S;
  const int tiles_x = (Ws + kBwdTile - 1) / kBwdTile, tiles_y = (Hs + kBwdTile - 1) / kBwdTile;
  const size_t tiles = (size_t)B * tiles_y * tiles_x;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {     // a block = one 16 x 16 tile of one source image
    const int x = (int)(t % tiles_x) * kBwdTile + (int)(threadIdx.x % kBwdTile);
    const int y = (int)((t / tiles_x) % tiles_y) * kBwdTile + (int)(threadIdx.x / kBwdTile);
    const int b = (int)(t / ((size_t)tiles_x * tiles_y));
    if (x >= Ws || y >= Hs) continue;
    float* dst = d_src + (size_t)b * 3 * src_plane + (size_t)y * Ws + x;     // channel c at dst[c * src_plane]
    float acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = first ? 0.f : dst[c * src_plane];
    for (int v = 0; v < nv; ++v) {
      const sgl_view& r = chunk.v[v];
      if (r.src != b || x < r.x0 || x >= r.x1 || y < r.y0 || y >= r.y1) continue;
      const ViewMap m = view_map(r);
      // cx = ax + axx X + axy Y, cy = ay + ayx X + ayy Y with (axx, ayy) or (axy, ayx) the +-1 pair: its own inverse
      const int dx = x - m.x0 - m.ax, dy = y - m.y0 - m.ay;
      const int X = m.axx != 0 ? dx * m.axx : dy * m.ayx;
      const int Y = m.axx != 0 ? dy * m.ayy : dx * m.axy;
      if (X < 0 || X >= m.ow || Y < 0 || Y >= m.oh) continue;   // kept canvas, w != h: this crop pixel was cut off
      const float* g = d_out + (size_t)v * 3 * plane;
      if (m.oh == S && m.ow == S) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += g[c * plane + (size_t)Y * S + X];
      } else {
        const AxisTables tb = axis_tables(scratch + tabs.off[v], m.oh, S);
        float f[3];
        bwd_filter_sum<3>(g, plane, tb, tb.ry[Y], tb.rx[X], Y, X, S, f);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += f[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * src_plane] = last ? acc[c] * inv_std : acc[c];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Adjoint of preprocess_aug_kernel<., float>(patch_major = 0) with respect to the source: the one non-linear transform
// of this file (clamps, a per-image mean, RGB <-> HSV).  Nothing of the forward is saved: a thread owns one output
// pixel, recomputes T = rotate(flip(resize(src))) (aug_geo) and the colour chain with the forward's own expressions,
// keeps the input of every operator in registers and walks the chain back.  Where the forward is not differentiable
// the rules are those of torch.autograd on oracle/preprocess_oracle.py: a clamp passes the gradient at its bounds
// (inclusive), max / min give it to the lowest channel index among ties, a where() differentiates the selected branch,
// floor / fmod / comparisons / the sector index contribute nothing.
//   aug_bwd_grey_kernel    the grey level in front of the contrast step, one thread per pixel: aug_mean_kernel's terms,
//                          stored in the not yet used d_T
//   aug_bwd_grey_mean_kernel   aug_mean_kernel's own sum over the stored terms, one block per image: the same additions in
//                          the same order, so m[b] has the forward's bits (tests/test_aug_bwd_gpu.py) and the recomputed
//                          chain clamps where the forward did, in 0.3 ms where the forward's pre-pass, whose one block
//                          per image also evaluates the terms, takes 7 ms (B = 128, 224 x 224 -> 384)
//   aug_bwd_colour<MEAN>   pass A: reverse the operators behind the contrast step, sum ghat = g [0 <= u <= 1] over the
//                          block's pixels and channels, one partial per block (wave_sum, then the four waves in order)
//   aug_bwd_fold_kernel    the partials of image b in a fixed order -> (sum ghat) / S^2, the contrast mean term
//   aug_bwd_colour<FULL>   pass B: the full reverse -> d_T; an image that is not rotated is stored straight into d_R
//                          (mirrored back when flipped: a permutation, one store per element)
//   aug_bwd_rotate_kernel  rotated images only, the transpose of the bilinear taps as a gather: an intermediate pixel u
//                          receives from the outputs whose sample point lies within one pixel of it, which are among
//                          the 5 x 5 outputs round M^T (u - ctr) + ctr (a rigid rotation needs 3 x 3: the sample points
//                          of the receivers lie within sqrt 2 of u).  Each candidate is tested with the forward's own
//                          floor and weights; taps outside the image never had a weight.  Order: oy, then ox
//   preprocess_bwd_kernel  d_R -> d_src, the resize adjoint above (tables, copy shortcut, the one multiply by 1 / std)
// No atomics, every sum in a fixed order, d_src written by one plain store per element.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool aug_in01(float u) { return u >= 0.f && u <= 1.f; }

// the vector-Jacobian product of aug_hue at c: g (cotangent of the result) -> cotangent of c, in place
__device__ __forceinline__ void aug_hue_bwd(const float* c, float shift, float* g) {
  const float r = c[0], gr = c[1], b = c[2];
  const float maxc = fmaxf(r, fmaxf(gr, b)), minc = fminf(r, fminf(gr, b));
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float d1 = eq ? 1.0f : maxc;
  const float sat = cr / d1;
  const float crd = eq ? 1.0f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - gr) / crd, bc = (maxc - b) / crd;
  const bool mr = maxc == r, mg = maxc == gr && maxc != r, mb = maxc != gr && maxc != r;
  const float hr = mr ? (bc - gc) : 0.f;
  const float hg = mg ? (2.0f + rc - bc) : 0.f;
  const float hb = mb ? (4.0f + gc - rc) : 0.f;
  float h = (hr + hg + hb) / 6.0f + 1.0f;
  h = h - floorf(h);
  h = h + shift;
  h = h - floorf(h);
  const float v = maxc;
  const float h6 = h * 6.0f;
  const float fi = floorf(h6);
  const float f = h6 - fi;
  const int i = (int)fi % 6;
  const float up = v * (1.0f - sat), uq = v * (1.0f - f * sat), ut = v * (1.0f - (1.0f - f) * sat);
  float gv = 0.f, gp = 0.f, gq = 0.f, gt = 0.f;
  switch (i) {
    case 0: gv = g[0]; gt = g[1]; gp = g[2]; break;
    case 1: gq = g[0]; gv = g[1]; gp = g[2]; break;
    case 2: gp = g[0]; gv = g[1]; gt = g[2]; break;
    case 3: gp = g[0]; gq = g[1]; gv = g[2]; break;
    case 4: gt = g[0]; gp = g[1]; gv = g[2]; break;
    default: gv = g[0]; gp = g[1]; gq = g[2]; break;
  }
  gp = aug_in01(up) ? gp : 0.f;
  gq = aug_in01(uq) ? gq : 0.f;
  gt = aug_in01(ut) ? gt : 0.f;
  float g_max = gv + gp * (1.0f - sat) + gq * (1.0f - f * sat) + gt * (1.0f - (1.0f - f) * sat);
  const float g_sat = -v * (gp + gq * f + gt * (1.0f - f));
  const float g_h = v * sat * (gt - gq);                 // f = 6 h - i and h = (hr + hg + hb) / 6 + ...: d f / d (hr + hg + hb) = 1
  float g_cr = g_sat / d1;
  if (!eq) g_max -= g_sat * sat / d1;
  float g_rc = 0.f, g_gc = 0.f, g_bc = 0.f;
  if (mr) g_bc += g_h, g_gc -= g_h;
  if (mg) g_rc += g_h, g_bc -= g_h;
  if (mb) g_gc += g_h, g_rc -= g_h;
  const float icrd = 1.0f / crd;
  g_max += (g_rc + g_gc + g_bc) * icrd;
  if (!eq) g_cr -= (g_rc * rc + g_gc * gc + g_bc * bc) * icrd;
  g_max += g_cr;
  const float g_min = -g_cr;
  const int imax = mr ? 0 : (maxc == gr ? 1 : 2);
  const int imin = minc == r ? 0 : (minc == gr ? 1 : 2);
  g[0] = -g_rc * icrd + (imax == 0 ? g_max : 0.f) + (imin == 0 ? g_min : 0.f);
  g[1] = -g_gc * icrd + (imax == 1 ? g_max : 0.f) + (imin == 1 ? g_min : 0.f);
  g[2] = -g_bc * icrd + (imax == 2 ? g_max : 0.f) + (imin == 2 ? g_min : 0.f);
}

// The colour chain forward from rgb = T (aug_colour_op, keeping every operator's input), then its reverse on g.  to_contrast: stop at the
// contrast step and return the sum over the channels of ghat (0 when the record has none); else g becomes the cotangent
// of T, with mean_term = (sum over the image of ghat) / S^2
__device__ __forceinline__ float aug_colour_bwd(const float* rgb, const AugSample& a, float grey_mean, float mean_term,
                                                bool to_contrast, float* g) {
  if (a.order[0] < 0) return 0.f;
  float x[4][3];
  float c[3] = {rgb[0], rgb[1], rgb[2]};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) x[k][ch] = c[ch];
    aug_colour_op(c, a, a.order[k], grey_mean);
  }
  const float w[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
  for (int k = 3; k >= 0; --k) {
    const int op = a.order[k];
    const float* xi = x[k];
    if (op == 0) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) g[ch] = aug_in01(xi[ch] * a.brightness) ? a.brightness * g[ch] : 0.f;
    } else if (op == 1) {
      float gh[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) gh[ch] = aug_in01((xi[ch] - grey_mean) * a.contrast + grey_mean) ? g[ch] : 0.f;
      if (to_contrast) return (gh[0] + gh[1]) + gh[2];
      const float m = (1.0f - a.contrast) * mean_term;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) g[ch] = a.contrast * gh[ch] + m * w[ch];
    } else if (op == 2) {
      const float gy = aug_grey(xi);
      float gh[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) gh[ch] = aug_in01((xi[ch] - gy) * a.saturation + gy) ? g[ch] : 0.f;
      const float s = (1.0f - a.saturation) * ((gh[0] + gh[1]) + gh[2]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) g[ch] = a.saturation * gh[ch] + s * w[ch];
    } else {
      aug_hue_bwd(xi, a.hue, g);
    }
  }
  return 0.f;
}

__device__ __forceinline__ bool aug_has_contrast(const AugSample& a) {
  bool need = false;
  if (a.order[0] >= 0)
    for (int k = 0; k < 4; ++k) need = need || a.order[k] == 1;
  return need;
}
__device__ __forceinline__ bool aug_rotates(const AugSample& a) { return !(a.sin_a == 0.f && a.cos_a == 1.f); }

// grey[b][p]: aug_mean_kernel's term of pixel p, for the images with a contrast step (the others' planes stay unwritten
// and unread).  Grid as aug_bwd_colour_kernel
template <bool SRC_U8>
__global__ __launch_bounds__(256) void aug_bwd_grey_kernel(const void* __restrict__ src, int Hs, int Ws, int S, int nblk,
                                                           const AugSample* __restrict__ aug, float* __restrict__ grey) {
  const int b = (int)(blockIdx.x / (unsigned)nblk);
  const size_t plane = (size_t)S * S;
  const size_t p = (size_t)(blockIdx.x % (unsigned)nblk) * 256 + threadIdx.x;
  const AugSample a = aug[b];
  if (!aug_has_contrast(a) || p >= plane) return;
  const float sy = (float)Hs / (float)S, sx = (float)Ws / (float)S;
  float rgb[3];
  aug_geo<SRC_U8>(src, b, (int)(p / S), (int)(p % S), Hs, Ws, S, sy, sx, a, rgb);
  aug_colour(rgb, a, 0.f, true);
  grey[(size_t)b * plane + p] = aug_grey(rgb);
}

// aug_mean_kernel with its terms read back: thread t adds pixels t, t + 256, ... in order, then the same tree
__global__ __launch_bounds__(256) void aug_bwd_grey_mean_kernel(const float* __restrict__ grey, int S,
                                                                const AugSample* __restrict__ aug,
                                                                float* __restrict__ grey_mean) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  if (!aug_has_contrast(aug[b])) {
    if (threadIdx.x == 0) grey_mean[b] = 0.f;
    return;
  }
  const size_t plane = (size_t)S * S;
  const float* g = grey + (size_t)b * plane;
  float acc = 0.f;
  for (size_t i = threadIdx.x; i < plane; i += 256) acc += g[i];
  acc = wave_sum(acc);
  if (lane_id() == 0) red[wave_id()] = acc;
  __syncthreads();
  if (threadIdx.x == 0) grey_mean[b] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)(S * S);
}

// Passes A (MEAN_PASS) and B.  grid: nblk = ceil(S^2 / 256) blocks per image, image b = blockIdx.x / nblk: a block never
// straddles two images.  A: partial[blockIdx.x] = the block's sum of ghat.  B: d_T (rotated images) or d_R (the others)
template <bool SRC_U8, bool MEAN_PASS>
__global__ __launch_bounds__(256) void aug_bwd_colour_kernel(const void* __restrict__ src,
                                                             const float* __restrict__ d_out, int Hs, int Ws, int S,
                                                             int nblk, const AugSample* __restrict__ aug,
                                                             const float* __restrict__ grey_mean,
                                                             const float* __restrict__ mean_term,
                                                             float* __restrict__ partial, float* __restrict__ d_T,
                                                             float* __restrict__ d_R) {
  __shared__ float red[4];
  const int b = (int)(blockIdx.x / (unsigned)nblk);
  const size_t plane = (size_t)S * S;
  const size_t p = (size_t)(blockIdx.x % (unsigned)nblk) * 256 + threadIdx.x;
  const AugSample a = aug[b];
  if (MEAN_PASS && !aug_has_contrast(a)) {               // block-uniform
    if (threadIdx.x == 0) partial[blockIdx.x] = 0.f;
    return;
  }
  const float sy = (float)Hs / (float)S, sx = (float)Ws / (float)S;
  float acc = 0.f;
  if (p < plane) {
    const int oy = (int)(p / S), ox = (int)(p % S);
    const float* go = d_out + (size_t)b * 3 * plane + p;
    float g[3] = {go[0], go[plane], go[2 * plane]};
    if (a.order[0] >= 0) {                               // the chain is the identity otherwise: nothing to recompute
      float rgb[3];
      aug_geo<SRC_U8>(src, b, oy, ox, Hs, Ws, S, sy, sx, a, rgb);
      acc = aug_colour_bwd(rgb, a, grey_mean[b], MEAN_PASS ? 0.f : mean_term[b], MEAN_PASS, g);
    }
    if (!MEAN_PASS) {
      const bool rot = aug_rotates(a);
      const int xr = (!rot && a.flip != 0.f) ? S - 1 - ox : ox;
      float* dst = (rot ? d_T : d_R) + (size_t)b * 3 * plane + (size_t)oy * S + xr;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) dst[ch * plane] = g[ch];
    }
  }
  if (MEAN_PASS) {
    acc = wave_sum(acc);
    if (lane_id() == 0) red[wave_id()] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// one block per image: mean_term[b] = (partial[b * nblk + 0 .. nblk) summed: thread t takes t, t + 256, ..., then the tree) / S^2
__global__ __launch_bounds__(256) void aug_bwd_fold_kernel(const float* __restrict__ partial, int nblk, int S,
                                                           float* __restrict__ mean_term) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  float acc = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[(size_t)b * nblk + i];
  acc = wave_sum(acc);
  if (lane_id() == 0) red[wave_id()] = acc;
  __syncthreads();
  if (threadIdx.x == 0) mean_term[b] = ((red[0] + red[1]) + (red[2] + red[3])) / ((float)S * (float)S);
}

// d_R[b] = flip^T rotate^T d_T[b] for the rotated images; the blocks of the others leave at once (pass B stored their d_R)
__global__ __launch_bounds__(256) void aug_bwd_rotate_kernel(const float* __restrict__ d_T, float* __restrict__ d_R, int S,
                                                             int nblk, const AugSample* __restrict__ aug) {
  const int b = (int)(blockIdx.x / (unsigned)nblk);
  const size_t plane = (size_t)S * S;
  const size_t p = (size_t)(blockIdx.x % (unsigned)nblk) * 256 + threadIdx.x;
  const AugSample a = aug[b];
  if (!aug_rotates(a) || p >= plane) return;
  const int uy = (int)(p / S), ux = (int)(p % S);
  const float ctr = 0.5f * (float)(S - 1);
  // the output whose sample point is u, up to rounding: o = M^T (u - ctr) + ctr
  const float du = (float)ux - ctr, dv = (float)uy - ctr;
  const float lim = (float)S + 4.0f;                      // keeps the window's integers small whatever the record holds
  const int cx = (int)rintf(fminf(fmaxf(a.cos_a * du + a.sin_a * dv + ctr, -4.0f), lim));
  const int cy = (int)rintf(fminf(fmaxf(a.cos_a * dv - a.sin_a * du + ctr, -4.0f), lim));
  const float* gT = d_T + (size_t)b * 3 * plane;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int oy = cy - 2; oy <= cy + 2; ++oy) {
    if (oy < 0 || oy >= S) continue;
    for (int ox = cx - 2; ox <= cx + 2; ++ox) {
      if (ox < 0 || ox >= S) continue;
      const float dx = (float)ox - ctr, dy = (float)oy - ctr;          // aug_geo's expressions from here on
      const float xs = a.cos_a * dx - a.sin_a * dy + ctr;
      const float ys = a.sin_a * dx + a.cos_a * dy + ctr;
      const float x0f = floorf(xs), y0f = floorf(ys);
      const int jx = ux - (int)x0f, jy = uy - (int)y0f;
      if (jx < 0 || jx > 1 || jy < 0 || jy > 1) continue;
      const float fx = xs - x0f, fy = ys - y0f;
      const float w = (jy ? fy : 1.0f - fy) * (jx ? fx : 1.0f - fx);
      if (w == 0.f) continue;
      const float* gp = gT + (size_t)oy * S + ox;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] += w * gp[ch * plane];
    }
  }
  float* dst = d_R + (size_t)b * 3 * plane + (size_t)uy * S + (a.flip != 0.f ? S - 1 - ux : ux);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) dst[ch * plane] = acc[ch];
}

// scratch of sgl_op_preprocess_aug_bwd: [resize tables][grey_mean B][mean_term B][partial B nblk][d_T B 3 S S][d_R B 3 S S]
struct AugBwdScratch {
  size_t tables, grey_mean, mean_term, partial, d_T, d_R, bytes;
  int nblk;
};
static AugBwdScratch aug_bwd_scratch(int B, int Hs, int Ws, int S) {
  AugBwdScratch s;
  const size_t plane = (size_t)S * S, img = (size_t)B * 3 * plane * sizeof(float);
  s.nblk = (int)((plane + 255) / 256);
  s.tables = 0;
  s.grey_mean = view_table_bytes(Hs, Ws, S);
  s.mean_term = s.grey_mean + (size_t)B * sizeof(float);
  s.partial = s.mean_term + (size_t)B * sizeof(float);
  s.d_T = s.partial + (size_t)B * s.nblk * sizeof(float);
  s.d_R = s.d_T + img;
  s.bytes = s.d_R + img;
  return s;
}

// the record checks sgl_op_preprocess_views and its adjoint share: SGL_OK, SGL_ERR_BAD_SHAPE or SGL_ERR_UNSUPPORTED
static int views_check(const sgl_view* rec, int V, int B, int Hs, int Ws, int S) {
  for (int v = 0; v < V; ++v) {
    const sgl_view& r = rec[v];
    if (!view_box_ok(r, B, Hs, Ws) || r.turns < 0 || r.turns > 3 || (r.keep_canvas | 1) != 1 || (r.flip | 1) != 1)
      return SGL_ERR_BAD_SHAPE;
  }
  for (int v = 0; v < V; ++v) {
    int oh, ow;
    view_extent(rec[v], &oh, &ow);
    if ((float)oh / (float)S > 16.f || (float)ow / (float)S > 16.f) return SGL_ERR_UNSUPPORTED;   // tap loops stay short
  }
  return SGL_OK;
}

// the argument checks every entry point shares, in the order in which refusals win: shape, patch geometry, output dtype,
// then (ratio: the source extents are what the filter reads) the 16x limit that keeps the tap loops short.  An entry point
// without an output layout passes patch_major = 0 and SGL_DTYPE_F32
static int check_args(int B, int Hs, int Ws, int S, float std, int patch_major, int P, int Kp, int out_dtype, bool ratio) {
  if (B <= 0 || Hs <= 0 || Ws <= 0 || S <= 0 || std == 0.f) return SGL_ERR_BAD_SHAPE;
  if (patch_major && (P <= 0 || S < P || Kp < 3 * P * P)) return SGL_ERR_BAD_SHAPE;
  if (out_dtype != SGL_DTYPE_BF16 && out_dtype != SGL_DTYPE_F16 && out_dtype != SGL_DTYPE_F32) return SGL_ERR_UNSUPPORTED;
  if (ratio && ((float)Hs / (float)S > 16.f || (float)Ws / (float)S > 16.f)) return SGL_ERR_UNSUPPORTED;
  return SGL_OK;
}

// f(std::bool_constant<source is uint8 NHWC>, (TOut*)out) for the six (source type, output dtype) pairs
template <typename F>
static void dispatch_src_out(int src_is_u8, int out_dtype, void* out, F&& f) {
  auto with_src = [&](auto u8) {
    if (out_dtype == SGL_DTYPE_BF16) f(u8, static_cast<bf16*>(out));
    else if (out_dtype == SGL_DTYPE_F16) f(u8, static_cast<f16*>(out));
    else f(u8, static_cast<float*>(out));
  };
  if (src_is_u8) with_src(std::true_type{});
  else with_src(std::false_type{});
}

static int capped_blocks(size_t total, int cap) {       // 256 threads per block, grid-stride above the cap
  const size_t blocks = (total + 255) / 256;
  return (int)(blocks < (size_t)cap ? blocks : (size_t)cap);
}

}  // namespace sgl

extern "C" {

int sgl_op_preprocess(const void* src, int src_is_u8_nhwc, int B, int Hs, int Ws, void* out, int out_dtype, int S, int P,
                      int Kp, int patch_major, float mean, float std, const int* mix_index, float lam,
                      sgl_stream stream) {
  if (!src || !out) return SGL_ERR_NULL;
  if (const int st = sgl::check_args(B, Hs, Ws, S, std, patch_major, P, Kp, out_dtype, true)) return st;
  const sgl::OutLayout L = {S, P, Kp, patch_major ? S / P : 0, patch_major};
  const int blocks = sgl::capped_blocks(L.elems(B), 16384);
  hipStream_t s = (hipStream_t)stream;
  const float inv_std = 1.0f / std;
  sgl::dispatch_src_out(src_is_u8_nhwc, out_dtype, out, [&](auto u8, auto* dst) {
    using T = std::remove_pointer_t<decltype(dst)>;
    hipLaunchKernelGGL((sgl::preprocess_kernel<decltype(u8)::value, T>), dim3(blocks), dim3(256), 0, s, src, dst, B, Hs, Ws,
                       L, mean, inv_std, mix_index, lam);
  });
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

size_t sgl_op_preprocess_views_scratch_bytes(int V, int S) {
  (void)V, (void)S;
  return 0;                                              // the records travel in the kernel arguments
}

int sgl_op_preprocess_views(const void* src, int src_is_u8_nhwc, int B, int Hs, int Ws, const sgl_view* views, int V,
                            void* out, int out_dtype, int S, int P, int Kp, int patch_major, float mean, float std,
                            void* scratch, size_t scratch_bytes, sgl_stream stream) {
  static_assert(sizeof(sgl::ViewChunk) <= 2048, "a chunk of records must fit the kernel arguments");
  if (!src || !views || !out) return SGL_ERR_NULL;
  if (V <= 0) return SGL_ERR_BAD_SHAPE;
  // a bad record is a bad shape and wins over a bad dtype, which wins over a record's unsupported ratio
  const int rec_status = sgl::views_check(views, V, B, Hs, Ws, S);
  if (rec_status == SGL_ERR_BAD_SHAPE) return rec_status;
  if (const int st = sgl::check_args(B, Hs, Ws, S, std, patch_major, P, Kp, out_dtype, false)) return st;
  if (rec_status != SGL_OK) return rec_status;
  if (scratch_bytes < sgl_op_preprocess_views_scratch_bytes(V, S)) return SGL_ERR_WORKSPACE;   // 0 bytes: never taken
  (void)scratch;
  const sgl::OutLayout L = {S, P, Kp, patch_major ? S / P : 0, patch_major};
  const size_t esize = out_dtype == SGL_DTYPE_F32 ? 4 : 2;
  hipStream_t s = (hipStream_t)stream;
  const float inv_std = 1.0f / std;
  for (int v0 = 0; v0 < V; v0 += sgl::kViewChunk) {      // one launch per 64 views
    const int nv = V - v0 < sgl::kViewChunk ? V - v0 : sgl::kViewChunk;
    sgl::ViewChunk chunk = {};
    for (int v = 0; v < nv; ++v) chunk.v[v] = views[v0 + v];
    const int blocks = sgl::capped_blocks(L.elems(nv), 4096);   // 256 CUs x 16, grid-stride
    if (blocks == 0) continue;                           // patch-major with S / P == 0 cannot happen (S >= P)
    sgl::dispatch_src_out(src_is_u8_nhwc, out_dtype, reinterpret_cast<char*>(out) + L.elems(v0) * esize,
                          [&](auto u8, auto* dst) {
      using T = std::remove_pointer_t<decltype(dst)>;
      hipLaunchKernelGGL((sgl::preprocess_views_kernel<decltype(u8)::value, T>), dim3(blocks), dim3(256), 0, s, src, dst,
                         chunk, nv, Hs, Ws, L, mean, inv_std);
    });
  }
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

size_t sgl_op_preprocess_views_bwd_scratch_bytes(const sgl_view* views, int V, int S) {
  if (!views || V <= 0 || S <= 0) return 0;
  size_t bytes = 0;
  for (int v = 0; v < V; ++v) {
    int oh, ow;
    sgl::view_extent(views[v], &oh, &ow);
    if (oh > 0 && ow > 0) bytes += sgl::view_table_bytes(oh, ow, S);   // an empty box is refused by the call itself
  }
  return bytes;
}

int sgl_op_preprocess_views_bwd(const float* d_out, int B, int Hs, int Ws, const sgl_view* views, int V, int S, float std,
                                float* d_src, void* scratch, size_t scratch_bytes, sgl_stream stream) {
  static_assert(sizeof(sgl::ViewChunk) + sizeof(sgl::ViewTableChunk) <= 3072, "records and offsets travel as arguments");
  static_assert(sizeof(sgl::AaAxis) % 4 == 0 && sizeof(sgl::SrcSpan) % 4 == 0, "tables stay 4-byte aligned");
  if (!d_out || !views || !d_src) return SGL_ERR_NULL;
  if (V <= 0 || (long long)34 * S > 0x7fffffffLL) return SGL_ERR_BAD_SHAPE;   // 2 S + oh + ow table entries in an int
  if (const int st = sgl::check_args(B, Hs, Ws, S, std, 0, 0, 0, SGL_DTYPE_F32, false)) return st;
  if (const int st = sgl::views_check(views, V, B, Hs, Ws, S)) return st;
  const size_t need = sgl_op_preprocess_views_bwd_scratch_bytes(views, V, S);
  if (need && !scratch) return SGL_ERR_NULL;
  if (scratch_bytes < need) return SGL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const size_t tiles = (size_t)B * ((Hs + sgl::kBwdTile - 1) / sgl::kBwdTile) * ((Ws + sgl::kBwdTile - 1) / sgl::kBwdTile);
  const int blocks = (int)(tiles < 8192 ? tiles : 8192);                               // 256 CUs x 32, grid-stride
  const float inv_std = 1.0f / std;
  size_t off = 0;
  for (int v0 = 0; v0 < V; v0 += sgl::kViewChunk) {      // one launch per 64 views, as the forward
    const int nv = V - v0 < sgl::kViewChunk ? V - v0 : sgl::kViewChunk;
    sgl::ViewChunk chunk = {};
    sgl::ViewTableChunk tabs = {};
    int entries = 0;                                     // the longest table of the chunk; 0: copies only
    for (int v = 0; v < nv; ++v) {
      chunk.v[v] = views[v0 + v];
      int oh, ow;
      sgl::view_extent(chunk.v[v], &oh, &ow);
      tabs.off[v] = off;
      const size_t bytes = sgl::view_table_bytes(oh, ow, S);
      off += bytes;
      if (bytes && 2 * S + oh + ow > entries) entries = 2 * S + oh + ow;
    }
    if (entries)
      hipLaunchKernelGGL(sgl::views_bwd_tables_kernel, dim3((unsigned)((entries + 255) / 256), (unsigned)nv), dim3(256), 0,
                         s, reinterpret_cast<char*>(scratch), chunk, tabs, S);
    hipLaunchKernelGGL(sgl::preprocess_views_bwd_kernel, dim3(blocks), dim3(256), 0, s,
                       d_out + (size_t)v0 * 3 * S * S, d_src, reinterpret_cast<char*>(scratch), chunk, tabs, nv, B, Hs, Ws,
                       S, (int)(v0 == 0), (int)(v0 + nv == V), inv_std);
  }
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

size_t sgl_op_preprocess_bwd_scratch_bytes(int B, int Hs, int Ws, int S) {
  if (B <= 0 || Hs <= 0 || Ws <= 0 || S <= 0) return 0;
  return sgl::view_table_bytes(Hs, Ws, S);
}

int sgl_op_preprocess_bwd(const float* d_out, int B, int Hs, int Ws, int S, float std, const int* mix_index, float lam,
                          float* d_src, void* scratch, size_t scratch_bytes, sgl_stream stream) {
  if (!d_out || !d_src) return SGL_ERR_NULL;
  if ((long long)2 * S + Hs + Ws > 0x7fffffffLL) return SGL_ERR_BAD_SHAPE;   // the tables' entries in an int
  if (const int st = sgl::check_args(B, Hs, Ws, S, std, 0, 0, 0, SGL_DTYPE_F32, true)) return st;   // the forward's limit
  const size_t need = sgl_op_preprocess_bwd_scratch_bytes(B, Hs, Ws, S);
  if (need && !scratch) return SGL_ERR_NULL;
  if (scratch_bytes < need) return SGL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  sgl::AxisTables t = {};
  if (need) {                                            // the tables of one view: the full frame, unturned, at offset 0
    t = sgl::axis_tables(reinterpret_cast<char*>(scratch), Hs, S);
    sgl::ViewChunk chunk = {};
    chunk.v[0] = sgl_view{0, 0, 0, Ws, Hs, 0, 0, 0};
    const int entries = 2 * S + Hs + Ws;
    hipLaunchKernelGGL(sgl::views_bwd_tables_kernel, dim3((unsigned)((entries + 255) / 256), 1u), dim3(256), 0, s,
                       reinterpret_cast<char*>(scratch), chunk, sgl::ViewTableChunk{}, S);
  }
  const int blocks = sgl::capped_blocks((size_t)B * 3 * Hs * Ws, 2048);   // 256 CUs x 8 blocks, grid-stride
  hipLaunchKernelGGL(sgl::preprocess_bwd_kernel, dim3(blocks), dim3(256), 0, s, d_out, d_src, B, Hs, Ws, S, 1.0f / std,
                     mix_index, lam, t);
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

int sgl_op_preprocess_aug(const void* src, int src_is_u8_nhwc, int B, int Hs, int Ws, void* out, int out_dtype, int S,
                          int P, int Kp, int patch_major, float mean, float std, const sgl_aug_sample* aug,
                          float* grey_mean, sgl_stream stream) {
  static_assert(sizeof(sgl_aug_sample) == sizeof(sgl::AugSample) && sizeof(sgl_aug_sample) == 48, "table layout");
  if (!src || !out || !aug || !grey_mean) return SGL_ERR_NULL;
  if (const int st = sgl::check_args(B, Hs, Ws, S, std, patch_major, P, Kp, out_dtype, true)) return st;
  hipStream_t s = (hipStream_t)stream;
  const sgl::AugSample* tab = reinterpret_cast<const sgl::AugSample*>(aug);
  if (src_is_u8_nhwc)
    hipLaunchKernelGGL((sgl::aug_mean_kernel<true>), dim3((unsigned)B), dim3(256), 0, s, src, Hs, Ws, S, tab, grey_mean);
  else
    hipLaunchKernelGGL((sgl::aug_mean_kernel<false>), dim3((unsigned)B), dim3(256), 0, s, src, Hs, Ws, S, tab, grey_mean);
  const sgl::OutLayout L = {S, P, Kp, patch_major ? S / P : 0, patch_major};
  const int side = patch_major ? L.g * P : S;
  const int blocks = sgl::capped_blocks((size_t)B * side * side, 16384);
  const float inv_std = 1.0f / std;
  sgl::dispatch_src_out(src_is_u8_nhwc, out_dtype, out, [&](auto u8, auto* dst) {
    using T = std::remove_pointer_t<decltype(dst)>;
    if (patch_major && Kp > 3 * P * P)
      hipLaunchKernelGGL((sgl::patch_pad_zero_kernel<T>), dim3(1024), dim3(256), 0, s, dst, (size_t)B * L.g * L.g, 3 * P * P,
                         Kp);
    hipLaunchKernelGGL((sgl::preprocess_aug_kernel<decltype(u8)::value, T>), dim3(blocks), dim3(256), 0, s, src, dst, B, Hs,
                       Ws, L, mean, inv_std, tab, grey_mean);
  });
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

size_t sgl_op_preprocess_aug_bwd_scratch_bytes(int B, int Hs, int Ws, int S) {
  if (B <= 0 || Hs <= 0 || Ws <= 0 || S <= 0) return 0;
  return sgl::aug_bwd_scratch(B, Hs, Ws, S).bytes;
}

int sgl_op_preprocess_aug_bwd(const float* d_out, const void* src, int src_is_u8_nhwc, int B, int Hs, int Ws, int S,
                              float std, const sgl_aug_sample* aug, float* d_src, void* scratch, size_t scratch_bytes,
                              sgl_stream stream) {
  if (!d_out || !src || !aug || !d_src || !scratch) return SGL_ERR_NULL;
  if (const int st = sgl::check_args(B, Hs, Ws, S, std, 0, 0, 0, SGL_DTYPE_F32, true)) return st;   // the forward's limit
  if ((long long)2 * S + Hs + Ws > 0x7fffffffLL) return SGL_ERR_BAD_SHAPE;   // the tables' entries in an int
  const sgl::AugBwdScratch L = sgl::aug_bwd_scratch(B, Hs, Ws, S);
  // B nblk is one block index; S * S stays an int, as in the forward's pre-pass
  if ((unsigned long long)B * (unsigned long long)L.nblk > 0x7fffffffULL || S > 46340) return SGL_ERR_BAD_SHAPE;
  if (scratch_bytes < L.bytes) return SGL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(scratch);
  float* grey_mean = reinterpret_cast<float*>(base + L.grey_mean);
  float* mean_term = reinterpret_cast<float*>(base + L.mean_term);
  float* partial = reinterpret_cast<float*>(base + L.partial);
  float* d_T = reinterpret_cast<float*>(base + L.d_T);
  float* d_R = reinterpret_cast<float*>(base + L.d_R);
  const sgl::AugSample* tab = reinterpret_cast<const sgl::AugSample*>(aug);
  const dim3 grid((unsigned)((size_t)B * L.nblk)), block(256);
  auto passes = [&](auto u8) {
    constexpr bool U8 = decltype(u8)::value;
    hipLaunchKernelGGL((sgl::aug_bwd_grey_kernel<U8>), grid, block, 0, s, src, Hs, Ws, S, L.nblk, tab, d_T);   // d_T is free
    hipLaunchKernelGGL(sgl::aug_bwd_grey_mean_kernel, dim3((unsigned)B), block, 0, s, d_T, S, tab, grey_mean);   // until pass B
    hipLaunchKernelGGL((sgl::aug_bwd_colour_kernel<U8, true>), grid, block, 0, s, src, d_out, Hs, Ws, S, L.nblk, tab,
                       grey_mean, mean_term, partial, d_T, d_R);
    hipLaunchKernelGGL(sgl::aug_bwd_fold_kernel, dim3((unsigned)B), block, 0, s, partial, L.nblk, S, mean_term);
    hipLaunchKernelGGL((sgl::aug_bwd_colour_kernel<U8, false>), grid, block, 0, s, src, d_out, Hs, Ws, S, L.nblk, tab,
                       grey_mean, mean_term, partial, d_T, d_R);
  };
  if (src_is_u8_nhwc) passes(std::true_type{});
  else passes(std::false_type{});
  hipLaunchKernelGGL(sgl::aug_bwd_rotate_kernel, grid, block, 0, s, d_T, d_R, S, L.nblk, tab);
  sgl::AxisTables t = {};
  if (sgl::view_table_bytes(Hs, Ws, S)) {                // as sgl_op_preprocess_bwd: the full frame's tables at offset 0
    t = sgl::axis_tables(base + L.tables, Hs, S);
    sgl::ViewChunk chunk = {};
    chunk.v[0] = sgl_view{0, 0, 0, Ws, Hs, 0, 0, 0};
    const int entries = 2 * S + Hs + Ws;
    hipLaunchKernelGGL(sgl::views_bwd_tables_kernel, dim3((unsigned)((entries + 255) / 256), 1u), block, 0, s, base, chunk,
                       sgl::ViewTableChunk{}, S);
  }
  const int blocks = sgl::capped_blocks((size_t)B * 3 * Hs * Ws, 2048);
  hipLaunchKernelGGL(sgl::preprocess_bwd_kernel, dim3(blocks), block, 0, s, d_R, d_src, B, Hs, Ws, S, 1.0f / std,
                     (const int*)nullptr, 1.0f, t);
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

}  // extern "C"
