// SID mask-decoder tail, second half of SURVEY.md §8f row 1 (Siglip2sidafrozen.py:731-745 decoder tail, :174-181 loss):
//
//   gate_mul       y = sigmoid(g) * x            the SE-style channel gate applied to the concatenated taps; one pass
//                  (dg, dx) from dy              instead of sigmoid + mul (and, backward, four elementwise kernels).
//                                                (B*N, E*K) bf16 at the default decoder: 525 MB per tensor at B = 64.
//   seg_loss_fwd   per-image partial sums of the BCE-with-logits and Dice terms of `bce_dice_loss` taken DIRECTLY from the
//                  low-resolution (B,1,g,g) logit map: every output pixel's logit is the bilinear (align_corners=False)
//                  interpolation of four low-res logits, evaluated in registers, so the (B,1,S,S) up-sampled logits are
//                  never written or read (147 k pixels per image; in the reference also the (B,512,S,S) features).
//   seg_loss_bwd   d loss / d low-res logits: the transposed bilinear interpolation of (p - t)/n + dice', gathered per
//                  low-res pixel in a fixed order (no atomics: bitwise reproducible).
//
// Loss definition being reproduced (heads.bce_dice_loss == Siglip2sidafrozen.py:174-181, on the images that carry a mask):
//   bce  = mean over all pixels of the selected images of  max(z,0) - z t + log(1 + exp(-|z|))
//   dice = 1 - mean_b( 2 sum(p t) / (sum p + sum t + eps) ),  p = sigmoid(z)
//   loss = bce_w * bce + dice_w * dice
//
//   seg_loss_ex    the same for `combined_segmentation_loss` (BCE + focal + Dice + boundary + IoU + smoothness), forward
//   _fwd / _bwd    and backward; described where it is defined, after seg_loss_bwd_kernel.
//
//   seg_eval       the validation half (Siglip2sidafrozen.py:183-240,1078-1106,1424-1569): per masked image, how many
//                  foreground / background pixels have their up-sampled logit between consecutive cut values, plus one
//                  4096-bin logit histogram per class for the pixel AUC.  Dice / IoU at any of the cuts, the threshold sweep
//                  and the AUC are all functions of those integer counts (heads.MaskMetrics); one read of the mask and of
//                  the g x g logits, integer atomics only (order-independent sums: bitwise reproducible), no host sync.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hip.h"
#include "kernels.h"
#include "siglip_hip.h"

namespace sgl {

__device__ __forceinline__ float sigmoidf_fast(float z) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-z * SGL_LOG2E));
}

template <typename T, int NV>
__global__ __launch_bounds__(256) void gate_mul_kernel(const T* __restrict__ g, const T* __restrict__ x,
                                                       T* __restrict__ y, size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    float a[NV], b[NV];
    Vec<T, NV>::ld(g + i * NV, a);
    Vec<T, NV>::ld(x + i * NV, b);
#pragma unroll
    for (int j = 0; j < NV; ++j) a[j] = sigmoidf_fast(a[j]) * b[j];
    Vec<T, NV>::st(y + i * NV, a);
  }
}

template <typename T, int NV>
__global__ __launch_bounds__(256) void gate_mul_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ g,
                                                           const T* __restrict__ x, T* __restrict__ dg,
                                                           T* __restrict__ dx, size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    float d[NV], a[NV], b[NV], og[NV], ox[NV];
    Vec<T, NV>::ld(dy + i * NV, d);
    Vec<T, NV>::ld(g + i * NV, a);
    Vec<T, NV>::ld(x + i * NV, b);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const float s = sigmoidf_fast(a[j]);
      ox[j] = d[j] * s;
      og[j] = d[j] * b[j] * (s * (1.0f - s));
    }
    if (dg) Vec<T, NV>::st(dg + i * NV, og);
    if (dx) Vec<T, NV>::st(dx + i * NV, ox);
  }
}

// bilinear source position of output index i (PyTorch upsample_bilinear2d, align_corners = False)
__device__ __forceinline__ void bil_src(int i, float scale, int g, int& i0, int& i1, float& w1) {
  float s = scale * ((float)i + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > g - 1) i0 = g - 1;
  i1 = i0 + 1 < g ? i0 + 1 : g - 1;
  w1 = s - (float)i0;
}

constexpr int SEG_ROWS = 8;   // output rows per block in the forward kernel

// partial[b][chunk][4] = { sum bce, sum p*t, sum p, sum t } over SEG_ROWS output rows of image b
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const float* __restrict__ lr /*[B][g][g]*/,
                                                           const float* __restrict__ tgt /*[B][S][S]*/,
                                                           float* __restrict__ partial, int g, int S, float scale,
                                                           int chunks) {
  __shared__ float red[4][4];
  const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
  const float* L = lr + (size_t)b * g * g;
  const float* T = tgt + (size_t)b * S * S;
  float s_bce = 0.f, s_pt = 0.f, s_p = 0.f, s_t = 0.f;
  const int r_begin = ch * SEG_ROWS, r_end = (r_begin + SEG_ROWS < S) ? r_begin + SEG_ROWS : S;
  for (int i = r_begin; i < r_end; ++i) {
    int y0, y1;
    float wy;
    bil_src(i, scale, g, y0, y1, wy);
    for (int j = threadIdx.x; j < S; j += 256) {
      int x0, x1;
      float wx;
      bil_src(j, scale, g, x0, x1, wx);
      const float top = L[y0 * g + x0] * (1.f - wx) + L[y0 * g + x1] * wx;
      const float bot = L[y1 * g + x0] * (1.f - wx) + L[y1 * g + x1] * wx;
      const float z = top * (1.f - wy) + bot * wy;
      const float t = T[(size_t)i * S + j];
      const float e = __expf(-fabsf(z));
      s_bce += fmaxf(z, 0.f) - z * t + log1pf(e);
      const float p = z >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
      s_pt += p * t;
      s_p += p;
      s_t += t;
    }
  }
  s_bce = wave_sum(s_bce); s_pt = wave_sum(s_pt); s_p = wave_sum(s_p); s_t = wave_sum(s_t);
  if (lane_id() == 0) {
    red[wave_id()][0] = s_bce; red[wave_id()][1] = s_pt; red[wave_id()][2] = s_p; red[wave_id()][3] = s_t;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    partial[((size_t)b * chunks + ch) * 4 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// One block per (image b, low-res row gy).  sums[b] = {sum bce, sum p t, sum p, sum t} of image b (forward output, folded);
// coef[b] = {c_bce, c_dice}: d loss / d z(pixel) = c_bce * (p - t) + c_dice * p (1-p) * ((2 t D - 2 I) / D^2) with
// I = sum p t, D = sum p + sum t + eps.  (c_bce = upstream * bce_w / n_pixels_total, c_dice = -upstream * dice_w / n_imgs;
// both 0 for images without a mask.)  dlr[b][gy][gx] = sum over output pixels of dz * bilinear weight: each thread owns
// output columns, sums them over the rows of the band in order, then one thread per gx folds its columns in order.
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ lr, const float* __restrict__ tgt,
                                                           const float* __restrict__ sums,
                                                           const float* __restrict__ coef, float* __restrict__ dlr,
                                                           int g, int S, float scale, float eps) {
  extern __shared__ float colacc[];   // [S][2]: contribution of output column j to (gy, x0(j)) and (gy, x1(j))
  const int b = blockIdx.x / g, gy = blockIdx.x - b * g;
  const float* L = lr + (size_t)b * g * g;
  const float* T = tgt + (size_t)b * S * S;
  const float c_bce = coef[2 * b], c_dice = coef[2 * b + 1];
  const float I = sums[4 * b + 1], D = sums[4 * b + 2] + sums[4 * b + 3] + eps;
  const float invD2 = 1.0f / (D * D);
  // output rows whose bilinear support can include gy (conservative range; exact test inside)
  const float inv = 1.0f / scale;
  int r_lo = (int)floorf(((float)gy - 1.0f + 0.5f) * inv - 0.5f) - 1;
  int r_hi = (int)ceilf(((float)gy + 1.0f + 0.5f) * inv - 0.5f) + 1;
  if (r_lo < 0) r_lo = 0;
  if (r_hi > S - 1) r_hi = S - 1;
  for (int j = threadIdx.x; j < S; j += 256) {
    int x0, x1;
    float wx;
    bil_src(j, scale, g, x0, x1, wx);
    float a0 = 0.f, a1 = 0.f;
    for (int i = r_lo; i <= r_hi; ++i) {
      int y0, y1;
      float wy;
      bil_src(i, scale, g, y0, y1, wy);
      const float wrow = (y0 == gy ? (1.f - wy) : 0.f) + (y1 == gy ? wy : 0.f);
      if (wrow == 0.f) continue;
      const float top = L[y0 * g + x0] * (1.f - wx) + L[y0 * g + x1] * wx;
      const float bot = L[y1 * g + x0] * (1.f - wx) + L[y1 * g + x1] * wx;
      const float z = top * (1.f - wy) + bot * wy;
      const float t = T[(size_t)i * S + j];
      const float e = __expf(-fabsf(z));
      const float p = z >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
      const float dz = c_bce * (p - t) + c_dice * (p * (1.f - p)) * ((2.f * t * D - 2.f * I) * invD2);
      a0 += dz * wrow * (1.f - wx);
      a1 += dz * wrow * wx;
    }
    colacc[2 * j] = a0;
    colacc[2 * j + 1] = a1;
  }
  __syncthreads();
  for (int gx = threadIdx.x; gx < g; gx += 256) {
    int c_lo = (int)floorf(((float)gx - 1.0f + 0.5f) * inv - 0.5f) - 1;
    int c_hi = (int)ceilf(((float)gx + 1.0f + 0.5f) * inv - 0.5f) + 1;
    if (c_lo < 0) c_lo = 0;
    if (c_hi > S - 1) c_hi = S - 1;
    float acc = 0.f;
    for (int j = c_lo; j <= c_hi; ++j) {
      int x0, x1;
      float wx;
      bil_src(j, scale, g, x0, x1, wx);
      // x0 == x1 at the right border: both halves belong to the same low-res pixel
      if (x0 == gx) acc += colacc[2 * j];
      if (x1 == gx) acc += colacc[2 * j + 1];
    }
    dlr[((size_t)b * g + gy) * g + gx] = acc;
  }
}

// ---- seg_loss_ex: combined_segmentation_loss ---------------------------------------------------------------------------
// The enhanced branch of the SID train step (Siglip2sidafrozen.py:69-172, heads.combined_segmentation_loss): BCE + focal +
// Dice + boundary-weighted BCE + IoU + the smoothness (total-variation) form of the morphological term, again straight from
// the low-resolution logits.  z, p and the BCE term of a pixel are formed as in seg_loss_fwd_kernel (seg_src below is the
// one difference, at most an ulp of z in the clamped last rows / columns); IoU needs no per-pixel sum of its own.  The three optional per-pixel computations are compiled in by TERMS:
//   SEG_FOCAL     alpha_t q^2 bce,  q = p + t - 2 p t,  alpha_t = alpha t + (1 - alpha)(1 - t)            (gamma = 2)
//   SEG_BOUNDARY  (1 + 3 beta) bce, beta = [s > 0] - [s == 9], s = the zero-padded 3x3 box sum of t (row-major order)
//   SEG_TV        |p[x+1] - p[x]| and |p[y+1] - p[y]|.  Every p is computed ONCE per row by seg_z / seg_p and staged in
//                 LDS, neighbours read it from there: two pixels whose taps and weights coincide (clamped borders, g = 1)
//                 hold the same bits, so their difference and its sign are exact zeros.
constexpr int SEG_FOCAL = SGL_SEG_TERM_FOCAL, SEG_BOUNDARY = SGL_SEG_TERM_BOUNDARY, SEG_TV = SGL_SEG_TERM_TV;
constexpr int SEG_EX_MAX_S = 2048;   // backward LDS: (2 + 4) rows of S floats = 48 KiB

// bil_src, with the weight taken as 0 where both taps are the same logit (the clamped last rows / columns): l (1 - w) + l w
// rounds differently for different w, and the smoothness term must see equal p there, as in exact arithmetic
__device__ __forceinline__ void seg_src(int i, float scale, int g, int& i0, int& i1, float& w1) {
  bil_src(i, scale, g, i0, i1, w1);
  if (i0 == i1) w1 = 0.f;
}

__device__ __forceinline__ float seg_z(const float* __restrict__ L, int g, int y0, int y1, float wy, int x0, int x1,
                                       float wx) {
  const float top = L[y0 * g + x0] * (1.f - wx) + L[y0 * g + x1] * wx;
  const float bot = L[y1 * g + x0] * (1.f - wx) + L[y1 * g + x1] * wx;
  return top * (1.f - wy) + bot * wy;
}

__device__ __forceinline__ float seg_p(float z, float e) { return z >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e); }

// dilate - erode of a {0,1} mask by the zero-padded 3x3 box (heads.boundary_aware_loss): -1 never occurs for such masks
__device__ __forceinline__ float seg_beta(const float* __restrict__ T, int S, int i, int j) {
  float s = 0.f;
#pragma unroll
  for (int di = -1; di <= 1; ++di)
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj) {
      const int y = i + di, x = j + dj;
      s += (y >= 0 && y < S && x >= 0 && x < S) ? T[(size_t)y * S + x] : 0.f;
    }
  return (s > 0.f ? 1.f : 0.f) - (s == 9.f ? 1.f : 0.f);
}

__device__ __forceinline__ float seg_sign(float a, float b) { return (a > b ? 1.f : 0.f) - (a < b ? 1.f : 0.f); }

// partial[b][chunk][8] = { sum bce, sum p*t, sum p, sum t, sum focal, sum boundary, sum |dp/dx|, sum |dp/dy| } over SEG_ROWS
// output rows of image b; the vertical pair (i, i + 1) belongs to the chunk of row i, so with SEG_TV a chunk also evaluates
// p (not the sums) of the row below its last one.  prow: three rows of p, so one barrier per row is enough.
template <int TERMS>
__global__ __launch_bounds__(256) void seg_loss_ex_fwd_kernel(const float* __restrict__ lr, const float* __restrict__ tgt,
                                                              float* __restrict__ partial, int g, int S, float scale,
                                                              int chunks, float alpha) {
  extern __shared__ float prow[];   // SEG_TV: [3][S]
  __shared__ float red[4][8];
  const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
  const float* L = lr + (size_t)b * g * g;
  const float* T = tgt + (size_t)b * S * S;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int r_begin = ch * SEG_ROWS, r_end = (r_begin + SEG_ROWS < S) ? r_begin + SEG_ROWS : S;
  const int r_last = ((TERMS & SEG_TV) && r_end < S) ? r_end : r_end - 1;
  for (int i = r_begin; i <= r_last; ++i) {
    int y0, y1;
    float wy;
    seg_src(i, scale, g, y0, y1, wy);
    const bool centre = i < r_end;
    float* cur = prow + (i % 3) * S;
    for (int j = threadIdx.x; j < S; j += 256) {
      int x0, x1;
      float wx;
      seg_src(j, scale, g, x0, x1, wx);
      const float z = seg_z(L, g, y0, y1, wy, x0, x1, wx);
      const float e = __expf(-fabsf(z));
      const float p = seg_p(z, e);
      if (TERMS & SEG_TV) cur[j] = p;
      if (centre) {
        const float t = T[(size_t)i * S + j];
        const float bce = fmaxf(z, 0.f) - z * t + log1pf(e);
        acc[0] += bce;
        acc[1] += p * t;
        acc[2] += p;
        acc[3] += t;
        if (TERMS & SEG_FOCAL) {
          const float q = (p + t) - 2.f * (p * t);
          const float at = alpha * t + (1.f - alpha) * (1.f - t);
          acc[4] += at * (q * q) * bce;
        }
        if (TERMS & SEG_BOUNDARY) acc[5] += (1.f + 3.f * seg_beta(T, S, i, j)) * bce;
      }
    }
    if (TERMS & SEG_TV) {
      __syncthreads();
      const float* prev = prow + ((i + 2) % 3) * S;
      for (int j = threadIdx.x; j < S; j += 256) {
        if (centre && j + 1 < S) acc[6] += fabsf(cur[j + 1] - cur[j]);
        if (i > r_begin) acc[7] += fabsf(cur[j] - prev[j]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    acc[k] = wave_sum(acc[k]);
    if (lane_id() == 0) red[wave_id()][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int k = threadIdx.x;
    partial[((size_t)b * chunks + ch) * 8 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// One block per (image b, low-res row gy), as seg_loss_bwd_kernel.  sums[b][8]: the folded forward sums (I = [1], P = [2],
// T = [3] are read); coef[b][6] = {c_bce, c_dice, c_focal, c_boundary, c_iou, c_tv}.  Per output pixel
//   dz = c_bce (p - t) + c_dice p(1-p) (2 t D - 2 I) / D^2 + c_focal alpha_t (2 q (1-2t) p(1-p) bce + q^2 (p - t))
//      + c_boundary (1 + 3 beta)(p - t) + c_iou p(1-p) (t U - I (1-t)) / U^2 + c_tv p(1-p) sum_nb sign(p - p_nb)
// with D = P + T + eps, U = P + T - I + smooth.  Rows are walked in order; with SEG_TV row i + 1 is staged (ring of four
// rows of p: one barrier per row) before row i is evaluated, and every p, the centre's included, is read from the ring.
// Each thread adds its columns' contributions into colacc in row order, then one thread per gx folds its columns in order.
template <int TERMS>
__global__ __launch_bounds__(256) void seg_loss_ex_bwd_kernel(const float* __restrict__ lr, const float* __restrict__ tgt,
                                                              const float* __restrict__ sums,
                                                              const float* __restrict__ coef, float* __restrict__ dlr,
                                                              int g, int S, float scale, float alpha, float eps,
                                                              float smooth) {
  extern __shared__ float colacc[];   // [S][2], then SEG_TV: ring [4][S]
  float* ring = colacc + 2 * S;
  const int b = blockIdx.x / g, gy = blockIdx.x - b * g;
  const float* L = lr + (size_t)b * g * g;
  const float* T = tgt + (size_t)b * S * S;
  const float c_bce = coef[6 * b], c_dice = coef[6 * b + 1], c_focal = coef[6 * b + 2], c_bnd = coef[6 * b + 3];
  const float c_iou = coef[6 * b + 4], c_tv = coef[6 * b + 5];
  const float I = sums[8 * b + 1], D = sums[8 * b + 2] + sums[8 * b + 3] + eps;
  const float U = (sums[8 * b + 2] + sums[8 * b + 3] - I) + smooth;
  const float invD2 = 1.0f / (D * D), invU2 = 1.0f / (U * U);
  const float inv = 1.0f / scale;
  int r_lo = (int)floorf(((float)gy - 1.0f + 0.5f) * inv - 0.5f) - 1;
  int r_hi = (int)ceilf(((float)gy + 1.0f + 0.5f) * inv - 0.5f) + 1;
  if (r_lo < 0) r_lo = 0;
  if (r_hi > S - 1) r_hi = S - 1;
  for (int j = threadIdx.x; j < S; j += 256) colacc[2 * j] = colacc[2 * j + 1] = 0.f;

  auto stage = [&](int i) {
    int y0, y1;
    float wy;
    seg_src(i, scale, g, y0, y1, wy);
    float* row = ring + (i & 3) * S;
    for (int j = threadIdx.x; j < S; j += 256) {
      int x0, x1;
      float wx;
      seg_src(j, scale, g, x0, x1, wx);
      const float z = seg_z(L, g, y0, y1, wy, x0, x1, wx);
      row[j] = seg_p(z, __expf(-fabsf(z)));
    }
  };
  if (TERMS & SEG_TV) {
    if (r_lo > 0) stage(r_lo - 1);
    stage(r_lo);
  }
  for (int i = r_lo; i <= r_hi; ++i) {
    if (TERMS & SEG_TV) {
      if (i + 1 < S) stage(i + 1);
      __syncthreads();
    }
    int y0, y1;
    float wy;
    seg_src(i, scale, g, y0, y1, wy);
    const float wrow = (y0 == gy ? (1.f - wy) : 0.f) + (y1 == gy ? wy : 0.f);
    if (wrow == 0.f) continue;
    const float* rc = ring + (i & 3) * S;
    const float* ru = ring + ((i + 3) & 3) * S;
    const float* rd = ring + ((i + 1) & 3) * S;
    for (int j = threadIdx.x; j < S; j += 256) {
      int x0, x1;
      float wx;
      seg_src(j, scale, g, x0, x1, wx);
      const float t = T[(size_t)i * S + j];
      float z = 0.f, e = 0.f, p;
      if (!(TERMS & SEG_TV) || (TERMS & SEG_FOCAL)) {
        z = seg_z(L, g, y0, y1, wy, x0, x1, wx);
        e = __expf(-fabsf(z));
      }
      if (TERMS & SEG_TV) p = rc[j];
      else p = seg_p(z, e);
      const float pq = p * (1.f - p), d = p - t;
      float dz = c_bce * d + c_dice * pq * ((2.f * t * D - 2.f * I) * invD2);
      dz += c_iou * pq * ((t * U - I * (1.f - t)) * invU2);
      if (TERMS & SEG_FOCAL) {
        const float bce = fmaxf(z, 0.f) - z * t + log1pf(e);
        const float q = (p + t) - 2.f * (p * t);
        const float at = alpha * t + (1.f - alpha) * (1.f - t);
        dz += c_focal * at * (2.f * q * (1.f - 2.f * t) * pq * bce + q * q * d);
      }
      if (TERMS & SEG_BOUNDARY) dz += c_bnd * (1.f + 3.f * seg_beta(T, S, i, j)) * d;
      if (TERMS & SEG_TV) {
        float sg = 0.f;
        if (i > 0) sg += seg_sign(p, ru[j]);
        if (i + 1 < S) sg += seg_sign(p, rd[j]);
        if (j > 0) sg += seg_sign(p, rc[j - 1]);
        if (j + 1 < S) sg += seg_sign(p, rc[j + 1]);
        dz += c_tv * pq * sg;
      }
      colacc[2 * j] += dz * wrow * (1.f - wx);
      colacc[2 * j + 1] += dz * wrow * wx;
    }
  }
  __syncthreads();
  for (int gx = threadIdx.x; gx < g; gx += 256) {
    int c_lo = (int)floorf(((float)gx - 1.0f + 0.5f) * inv - 0.5f) - 1;
    int c_hi = (int)ceilf(((float)gx + 1.0f + 0.5f) * inv - 0.5f) + 1;
    if (c_lo < 0) c_lo = 0;
    if (c_hi > S - 1) c_hi = S - 1;
    float acc = 0.f;
    for (int j = c_lo; j <= c_hi; ++j) {
      int x0, x1;
      float wx;
      seg_src(j, scale, g, x0, x1, wx);
      if (x0 == gx) acc += colacc[2 * j];
      if (x1 == gx) acc += colacc[2 * j + 1];
    }
    dlr[((size_t)b * g + gy) * g + gx] = acc;
  }
}

// ---- seg_eval ----------------------------------------------------------------------------------------------------------
// One block per (image, band of SEG_EVAL_ROWS output rows).  A band is one contiguous run of mask elements, so it is walked
// as a flat array: scalar elements up to the first 16-byte boundary, 16-byte vectors (4 floats / 16 bytes of mask), a scalar
// tail; any element alignment of the mask works.  Counters live in LDS (32-bit: a band has < 2^31 pixels) and are flushed
// once per block, non-zero bins only, consecutive lanes to consecutive bins: up-sampled logits are smooth, so the bins a
// band touches are a few contiguous runs.  The per-cut histogram has only K+1 bins per class (a wave's 64 lanes would pile
// onto two or three addresses), so it is kept in SEG_EVAL_COPIES copies indexed by lane.
constexpr int SEG_EVAL_ROWS = 64;
constexpr int SEG_EVAL_COPIES = 8;
constexpr int SEG_EVAL_KMAX = 64;
constexpr int SEG_EVAL_NB = SGL_SEG_EVAL_AUC_BINS;

template <bool AUC>
__device__ __forceinline__ void seg_eval_count(float z, int c, const float* cs, int* hl, unsigned* al) {
  // k = number of cuts strictly below z (cs is padded to 64 entries with +inf; NaN compares false: k = 0)
  int k = 0;
#pragma unroll
  for (int step = SEG_EVAL_KMAX; step > 0; step >>= 1)
    if (k + step <= SEG_EVAL_KMAX && cs[k + step - 1] < z) k += step;
  atomicAdd(&hl[c * (SEG_EVAL_KMAX + 1) + k], 1);
  if (AUC) {
    const float f = (z + 16.0f) * ((float)SEG_EVAL_NB / 32.0f);
    int bin = 0;                                                 // NaN and everything below -16
    if (f >= 0.0f) bin = f < (float)SEG_EVAL_NB ? (int)f : SEG_EVAL_NB - 1;
    atomicAdd(&al[c * SEG_EVAL_NB + bin], 1u);
  }
}

__device__ __forceinline__ int seg_eval_class(float t) { return t > 0.5f ? 1 : 0; }
__device__ __forceinline__ int seg_eval_class(uint8_t t) { return t ? 1 : 0; }      // an integer above 0.5 is one that is not 0

template <typename TT, bool AUC>
__global__ __launch_bounds__(256) void seg_eval_kernel(const float* __restrict__ lr /*[B][g][g]*/,
                                                       const TT* __restrict__ tgt /*[B][S][S]*/,
                                                       const uint8_t* __restrict__ sel, const float* __restrict__ cuts,
                                                       int K, int32_t* __restrict__ hist,
                                                       unsigned long long* __restrict__ auc, int g, int S, float scale,
                                                       int bands) {
  constexpr int VEC = 16 / (int)sizeof(TT);
  constexpr int HL = 2 * (SEG_EVAL_KMAX + 1);
  __shared__ float cs[SEG_EVAL_KMAX];
  __shared__ int hl[SEG_EVAL_COPIES][HL];
  __shared__ unsigned al[AUC ? 2 * SEG_EVAL_NB : 1];
  const int b = blockIdx.x / bands, band = blockIdx.x - b * bands;
  if (sel && !sel[b]) return;                                    // its hist row was zeroed by the entry point
  const int tid = threadIdx.x;
  if (tid < SEG_EVAL_KMAX) cs[tid] = tid < K ? cuts[tid] : __builtin_inff();
  for (int i = tid; i < SEG_EVAL_COPIES * HL; i += 256) (&hl[0][0])[i] = 0;
  if (AUC)
    for (int i = tid; i < 2 * SEG_EVAL_NB; i += 256) al[i] = 0u;
  __syncthreads();

  const float* L = lr + (size_t)b * g * g;
  const int r0 = band * SEG_EVAL_ROWS, r1 = r0 + SEG_EVAL_ROWS < S ? r0 + SEG_EVAL_ROWS : S;
  const TT* P = tgt + (size_t)b * S * S + (size_t)r0 * S;        // the band: n contiguous elements
  const int n = (r1 - r0) * S;
  int head = (int)(((16u - (unsigned)((uintptr_t)P & 15u)) & 15u) / (unsigned)sizeof(TT));
  if (head > n) head = n;
  const int nvec = (n - head) / VEC;
  int* myh = hl[tid & (SEG_EVAL_COPIES - 1)];

  auto pixel = [&](int i, int j, int c) {                        // i: output row (absolute), j: output column
    int y0, y1, x0, x1;
    float wy, wx;
    bil_src(i, scale, g, y0, y1, wy);
    bil_src(j, scale, g, x0, x1, wx);
    const float top = L[y0 * g + x0] * (1.f - wx) + L[y0 * g + x1] * wx;
    const float bot = L[y1 * g + x0] * (1.f - wx) + L[y1 * g + x1] * wx;
    const float z = top * (1.f - wy) + bot * wy;
    seg_eval_count<AUC>(z, c, cs, myh, al);
  };

  for (int v = tid; v < nvec; v += 256) {
    const int idx = head + v * VEC;
    alignas(16) TT t[VEC];
    *reinterpret_cast<uint4*>(t) = *reinterpret_cast<const uint4*>(P + idx);
    int i = idx / S, j = idx - i * S;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      pixel(r0 + i, j, seg_eval_class(t[e]));
      if (++j == S) { j = 0; ++i; }
    }
  }
  const int rest = n - nvec * VEC;                               // head + tail scalars, fewer than 2 * VEC
  for (int t = tid; t < rest; t += 256) {
    const int idx = t < head ? t : nvec * VEC + t;
    const int i = idx / S, j = idx - i * S;
    pixel(r0 + i, j, seg_eval_class(P[idx]));
  }
  __syncthreads();

  for (int i = tid; i < 2 * (K + 1); i += 256) {
    const int c = i / (K + 1), k = i - c * (K + 1);
    int v = 0;
#pragma unroll
    for (int q = 0; q < SEG_EVAL_COPIES; ++q) v += hl[q][c * (SEG_EVAL_KMAX + 1) + k];
    if (v) atomicAdd(&hist[((size_t)b * 2 + c) * (K + 1) + k], v);
  }
  if (AUC)
    for (int i = tid; i < 2 * SEG_EVAL_NB; i += 256) {
      const unsigned v = al[i];
      if (v) atomicAdd(&auc[i], (unsigned long long)v);
    }
}

}  // namespace sgl

extern "C" {

int sgl_op_gate_mul(const void* g, const void* x, void* y, size_t n, int dtype, sgl_stream stream) {
  if (!g || !x || !y) return SGL_ERR_NULL;
  if (dtype != SGL_DTYPE_BF16 && dtype != SGL_DTYPE_F32) return SGL_ERR_UNSUPPORTED;
  const int nv = dtype == SGL_DTYPE_BF16 ? 8 : 4;
  if (n % nv || ((((uintptr_t)g) | ((uintptr_t)x) | ((uintptr_t)y)) & 15)) return SGL_ERR_BAD_SHAPE;
  const size_t nvec = n / nv;
  if (nvec == 0) return SGL_OK;
  const int blocks = (int)((nvec + 255) / 256 < 8192 ? (nvec + 255) / 256 : 8192);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SGL_DTYPE_BF16)
    hipLaunchKernelGGL((sgl::gate_mul_kernel<sgl::bf16, 8>), dim3(blocks), dim3(256), 0, s, (const sgl::bf16*)g,
                       (const sgl::bf16*)x, (sgl::bf16*)y, nvec);
  else
    hipLaunchKernelGGL((sgl::gate_mul_kernel<float, 4>), dim3(blocks), dim3(256), 0, s, (const float*)g, (const float*)x,
                       (float*)y, nvec);
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

int sgl_op_gate_mul_bwd(const void* dy, const void* g, const void* x, void* dg, void* dx, size_t n, int dtype,
                        sgl_stream stream) {
  if (!dy || !g || !x) return SGL_ERR_NULL;
  if (dtype != SGL_DTYPE_BF16 && dtype != SGL_DTYPE_F32) return SGL_ERR_UNSUPPORTED;
  const int nv = dtype == SGL_DTYPE_BF16 ? 8 : 4;
  if (n % nv || ((((uintptr_t)dy) | ((uintptr_t)g) | ((uintptr_t)x) | ((uintptr_t)dg) | ((uintptr_t)dx)) & 15))
    return SGL_ERR_BAD_SHAPE;
  const size_t nvec = n / nv;
  if (nvec == 0) return SGL_OK;
  const int blocks = (int)((nvec + 255) / 256 < 8192 ? (nvec + 255) / 256 : 8192);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SGL_DTYPE_BF16)
    hipLaunchKernelGGL((sgl::gate_mul_bwd_kernel<sgl::bf16, 8>), dim3(blocks), dim3(256), 0, s, (const sgl::bf16*)dy,
                       (const sgl::bf16*)g, (const sgl::bf16*)x, (sgl::bf16*)dg, (sgl::bf16*)dx, nvec);
  else
    hipLaunchKernelGGL((sgl::gate_mul_bwd_kernel<float, 4>), dim3(blocks), dim3(256), 0, s, (const float*)dy,
                       (const float*)g, (const float*)x, (float*)dg, (float*)dx, nvec);
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

int sgl_op_seg_loss_chunks(int S) { return S > 0 ? (S + sgl::SEG_ROWS - 1) / sgl::SEG_ROWS : 0; }

int sgl_op_seg_loss_fwd(const float* logits_lr, const float* targets, float* partial, int B, int g, int S,
                        sgl_stream stream) {
  if (!logits_lr || !targets || !partial) return SGL_ERR_NULL;
  if (B <= 0 || g <= 0 || S <= 0 || g > 4096 || S > 16384) return SGL_ERR_BAD_SHAPE;
  const int chunks = sgl_op_seg_loss_chunks(S);
  hipLaunchKernelGGL(sgl::seg_loss_fwd_kernel, dim3((unsigned)(B * chunks)), dim3(256), 0, (hipStream_t)stream, logits_lr,
                     targets, partial, g, S, (float)g / (float)S, chunks);
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

int sgl_op_seg_loss_bwd(const float* logits_lr, const float* targets, const float* sums, const float* coef,
                        float* dlogits_lr, int B, int g, int S, float eps, sgl_stream stream) {
  if (!logits_lr || !targets || !sums || !coef || !dlogits_lr) return SGL_ERR_NULL;
  if (B <= 0 || g <= 0 || S <= 0 || g > 4096 || S > 8192) return SGL_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(sgl::seg_loss_bwd_kernel, dim3((unsigned)(B * g)), dim3(256), (size_t)S * 2 * sizeof(float),
                     (hipStream_t)stream, logits_lr, targets, sums, coef, dlogits_lr, g, S, (float)g / (float)S, eps);
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

static int seg_loss_ex_check(int B, int g, int S, int terms) {
  if (B <= 0 || g <= 0 || S < 2 || g > 4096 || S > sgl::SEG_EX_MAX_S) return SGL_ERR_BAD_SHAPE;
  if ((long long)B * sgl_op_seg_loss_chunks(S) > 0x7fffffffLL || (long long)B * g > 0x7fffffffLL) return SGL_ERR_BAD_SHAPE;
  if (terms & ~(SGL_SEG_TERM_FOCAL | SGL_SEG_TERM_BOUNDARY | SGL_SEG_TERM_TV)) return SGL_ERR_UNSUPPORTED;
  return SGL_OK;
}

// one launch of KERNEL<terms> for terms in 0..7
#define SEG_EX_LAUNCH(KERNEL, GRID, LDS, ...)                                                                              \
  switch (terms) {                                                                                                         \
    case 0: hipLaunchKernelGGL((sgl::KERNEL<0>), GRID, dim3(256), LDS, (hipStream_t)stream, __VA_ARGS__); break;           \
    case 1: hipLaunchKernelGGL((sgl::KERNEL<1>), GRID, dim3(256), LDS, (hipStream_t)stream, __VA_ARGS__); break;           \
    case 2: hipLaunchKernelGGL((sgl::KERNEL<2>), GRID, dim3(256), LDS, (hipStream_t)stream, __VA_ARGS__); break;           \
    case 3: hipLaunchKernelGGL((sgl::KERNEL<3>), GRID, dim3(256), LDS, (hipStream_t)stream, __VA_ARGS__); break;           \
    case 4: hipLaunchKernelGGL((sgl::KERNEL<4>), GRID, dim3(256), LDS, (hipStream_t)stream, __VA_ARGS__); break;           \
    case 5: hipLaunchKernelGGL((sgl::KERNEL<5>), GRID, dim3(256), LDS, (hipStream_t)stream, __VA_ARGS__); break;           \
    case 6: hipLaunchKernelGGL((sgl::KERNEL<6>), GRID, dim3(256), LDS, (hipStream_t)stream, __VA_ARGS__); break;           \
    default: hipLaunchKernelGGL((sgl::KERNEL<7>), GRID, dim3(256), LDS, (hipStream_t)stream, __VA_ARGS__); break;          \
  }

int sgl_op_seg_loss_ex_fwd(const float* logits_lr, const float* targets, float* partial, int B, int g, int S, int terms,
                           float alpha, sgl_stream stream) {
  if (!logits_lr || !targets || !partial) return SGL_ERR_NULL;
  if (const int st = seg_loss_ex_check(B, g, S, terms)) return st;
  const int chunks = sgl_op_seg_loss_chunks(S);
  const size_t lds = (terms & SGL_SEG_TERM_TV) ? (size_t)S * 3 * sizeof(float) : 0;
  SEG_EX_LAUNCH(seg_loss_ex_fwd_kernel, dim3((unsigned)(B * chunks)), lds, logits_lr, targets, partial, g, S,
                (float)g / (float)S, chunks, alpha)
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

int sgl_op_seg_loss_ex_bwd(const float* logits_lr, const float* targets, const float* sums, const float* coef,
                           float* dlogits_lr, int B, int g, int S, int terms, float alpha, float eps, float smooth,
                           sgl_stream stream) {
  if (!logits_lr || !targets || !sums || !coef || !dlogits_lr) return SGL_ERR_NULL;
  if (const int st = seg_loss_ex_check(B, g, S, terms)) return st;
  const size_t lds = (size_t)S * ((terms & SGL_SEG_TERM_TV) ? 6 : 2) * sizeof(float);
  SEG_EX_LAUNCH(seg_loss_ex_bwd_kernel, dim3((unsigned)(B * g)), lds, logits_lr, targets, sums, coef, dlogits_lr, g, S,
                (float)g / (float)S, alpha, eps, smooth)
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}
#undef SEG_EX_LAUNCH

int sgl_op_seg_eval_auc_bins(void) { return SGL_SEG_EVAL_AUC_BINS; }

int sgl_op_seg_eval(const float* logits_lr, const void* targets, int target_dtype, const uint8_t* sel, const float* cuts,
                    int K, int32_t* hist, unsigned long long* auc_hist, int B, int g, int S, sgl_stream stream) {
  if (!logits_lr || !targets || !cuts || !hist) return SGL_ERR_NULL;
  if (B <= 0 || g <= 0 || S <= 0 || K < 1 || K > sgl::SEG_EVAL_KMAX || S > 32768 || g > 32768) return SGL_ERR_BAD_SHAPE;
  if (target_dtype != SGL_DTYPE_F32 && target_dtype != SGL_DTYPE_U8) return SGL_ERR_UNSUPPORTED;
  if (target_dtype == SGL_DTYPE_F32 && ((uintptr_t)targets & 3)) return SGL_ERR_BAD_SHAPE;
  const int bands = (S + sgl::SEG_EVAL_ROWS - 1) / sgl::SEG_EVAL_ROWS;
  if ((long long)B * bands > 0x7fffffffLL) return SGL_ERR_BAD_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, (size_t)B * 2 * (K + 1) * sizeof(int32_t), s) != hipSuccess) return SGL_ERR_HIP;
  const dim3 grid((unsigned)(B * bands)), block(256);
  const float scale = (float)g / (float)S;
  if (target_dtype == SGL_DTYPE_F32) {
    if (auc_hist)
      hipLaunchKernelGGL((sgl::seg_eval_kernel<float, true>), grid, block, 0, s, logits_lr, (const float*)targets, sel, cuts,
                         K, hist, auc_hist, g, S, scale, bands);
    else
      hipLaunchKernelGGL((sgl::seg_eval_kernel<float, false>), grid, block, 0, s, logits_lr, (const float*)targets, sel, cuts,
                         K, hist, auc_hist, g, S, scale, bands);
  } else {
    if (auc_hist)
      hipLaunchKernelGGL((sgl::seg_eval_kernel<uint8_t, true>), grid, block, 0, s, logits_lr, (const uint8_t*)targets, sel,
                         cuts, K, hist, auc_hist, g, S, scale, bands);
    else
      hipLaunchKernelGGL((sgl::seg_eval_kernel<uint8_t, false>), grid, block, 0, s, logits_lr, (const uint8_t*)targets, sel,
                         cuts, K, hist, auc_hist, g, S, scale, bands);
  }
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

}  // extern "C"
