// HBM-bound helper kernels around the encoder GEMMs (gfx950): patch gather (im2col), weight-shadow casts,
// bias-gradient column sums, position-table bicubic resize, and the 1-query attention-pool head.
#include "common.hip.h"
#include "shadow_tile.hip.h"
#include "kernels.h"

namespace sgl {

// ---- im2col: Conv2d(3->D, k=s=P, 'valid') becomes a GEMM over K = 3*P*P (TF:modeling_siglip.py:124-130,178).
// out[m][k], m = (b, gy, gx), k = c*P*P + ky*P + kx  (== weight.reshape(D,-1) order); k >= 3P² is zero pad.
template <typename T>
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ pix, int channels_last,
                                                     T* __restrict__ out, int B, int H, int W, int P, int gh, int gw,
                                                     int Kp) {
  const size_t total = (size_t)B * gh * gw * Kp;
  const int K = 3 * P * P;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int k = (int)(idx % Kp);
    const size_t m = idx / Kp;
    float v = 0.f;
    if (k < K) {
      const int gx = (int)(m % gw);
      const int gy = (int)((m / gw) % gh);
      const int b = (int)(m / ((size_t)gw * gh));
      const int c = k / (P * P);
      const int r = k - c * P * P;
      const int ky = r / P, kx = r - ky * P;
      const int yy = gy * P + ky, xx = gx * P + kx;
      const size_t src = channels_last ? (((size_t)b * H + yy) * W + xx) * 3 + c
                                       : (((size_t)b * 3 + c) * H + yy) * W + xx;
      v = pix[src];
    }
    Elem<T>::st(out + idx, v);
  }
}

hipError_t im2col(const float* pix, int channels_last, void* out, int out_dtype, int B, int H, int W, int P, int Kp,
                  hipStream_t s) {
  const int gh = H / P, gw = W / P;
  const size_t total = (size_t)B * gh * gw * Kp;
  if (total == 0) return hipSuccess;
  int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  if (out_dtype == DT_BF16)
    hipLaunchKernelGGL(im2col_kernel<bf16>, dim3(blocks), dim3(256), 0, s, pix, channels_last, (bf16*)out, B, H, W, P,
                       gh, gw, Kp);
  else if (out_dtype == DT_F16)
    hipLaunchKernelGGL(im2col_kernel<f16>, dim3(blocks), dim3(256), 0, s, pix, channels_last, (f16*)out, B, H, W, P,
                       gh, gw, Kp);
  else
    hipLaunchKernelGGL(im2col_kernel<float>, dim3(blocks), dim3(256), 0, s, pix, channels_last, (float*)out, B, H, W,
                       P, gh, gw, Kp);
  return hipGetLastError();
}

// ---- col2im: the adjoint of im2col.  d_pixels[b][c][y][x] = d_cols[(b, y / P, x / P)][c*P*P + (y % P)*P + x % P] for
// y < gh*P and x < gw*P, exact zero on the trailing rows / columns the 'valid' convolution never reads.  Patches do not
// overlap, so every pixel has one source: a gather, no atomics, bitwise reproducible.  Columns >= 3*P*P of d_cols are never
// read.  One thread writes V consecutive floats of one pixel row of the output (row = W floats in NCHW, 3*W in NHWC):
// V = 4 (one 16-byte store) when the row length is a multiple of 4, and the four sources are one 16-byte load when they
// are four consecutive kx of one patch (NCHW, P % 4 == 0); otherwise four 4-byte loads.  HBM-bound: 4 B read + 4 B written
// per pixel.  Index decode: one 64-bit divide per thread (group -> pixel row); the row number (< 2^31, checked by the
// launcher) and everything inside the row are 32-bit.
template <int V>
__global__ __launch_bounds__(256) void col2im_kernel(const float* __restrict__ dc, float* __restrict__ dpix,
                                                     int channels_last, int H, int W, int P, int gh, int gw, int Kp,
                                                     int vec_src, size_t groups, unsigned gpr) {
  const unsigned rowlen = gpr * V;   // floats per pixel row of the output
  const unsigned PP = (unsigned)(P * P);
  for (size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * 256) {
    const unsigned row = (unsigned)(gi / gpr);
    const unsigned e0 = (unsigned)(gi - (size_t)row * gpr) * V;   // first float of the group within its row
    // NCHW: row = (b*3 + c)*H + y;  NHWC: row = b*H + y
    const unsigned q = row / (unsigned)H, y = row - q * (unsigned)H;
    const unsigned b = channels_last ? q : q / 3u, c0 = channels_last ? 0u : q - b * 3u;
    const unsigned gy = y / (unsigned)P, ky = y - gy * (unsigned)P;
    const bool row_ok = gy < (unsigned)gh;
    // the ky-th row of patch (b, gy, 0), channel 0; patch gx is gx*Kp further, channel c is c*P*P further
    const float* src = dc + ((size_t)b * gh + gy) * gw * Kp + ky * (unsigned)P;
    float* dst = dpix + (size_t)row * rowlen + e0;
    float v[V];
    if (V == 4 && vec_src) {   // NCHW, P % 4 == 0, W % 4 == 0: x % 4 == 0, so the four pixels are kx .. kx + 3 of one patch row
      const unsigned gx = e0 / (unsigned)P, kx = e0 - gx * (unsigned)P;
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (row_ok && gx < (unsigned)gw) t = *reinterpret_cast<const f32x4*>(src + (size_t)gx * Kp + c0 * PP + kx);
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = t[j];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const unsigned e = e0 + j;
        const unsigned x = channels_last ? e / 3u : e, c = channels_last ? e - x * 3u : c0;
        const unsigned gx = x / (unsigned)P, kx = x - gx * (unsigned)P;
        v[j] = (row_ok && gx < (unsigned)gw) ? src[(size_t)gx * Kp + c * PP + kx] : 0.f;
      }
    }
    if constexpr (V == 4) {
      *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
      dst[0] = v[0];
    }
  }
}

hipError_t col2im(const float* d_cols, int B, int H, int W, int P, int Kp, float* d_pixels, int channels_last,
                  hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0 || P <= 0 || Kp < 3 * P * P || (channels_last != 0 && channels_last != 1))
    return hipErrorInvalidValue;
  const int gh = H / P, gw = W / P;
  const size_t rows = (size_t)B * H * (channels_last ? 1 : 3);
  const size_t rowlen = (size_t)W * (channels_last ? 3 : 1);
  if (rows >= (1ull << 31) || rowlen >= (1ull << 31)) return hipErrorInvalidValue;   // 32-bit row arithmetic in the kernel
  const bool v4 = (rowlen % 4) == 0 && (((uintptr_t)d_pixels) & 15) == 0;
  const int vec_src = v4 && !channels_last && (P % 4) == 0 && (Kp % 4) == 0 && (((uintptr_t)d_cols) & 15) == 0;
  const unsigned gpr = (unsigned)(v4 ? rowlen / 4 : rowlen);   // groups per row
  const size_t groups = rows * gpr;
  const int blocks = (int)((groups + 255) / 256 < 16384 ? (groups + 255) / 256 : 16384);
  if (v4)
    hipLaunchKernelGGL(col2im_kernel<4>, dim3(blocks), dim3(256), 0, s, d_cols, d_pixels, channels_last, H, W, P, gh, gw, Kp,
                       vec_src, groups, gpr);
  else
    hipLaunchKernelGGL(col2im_kernel<1>, dim3(blocks), dim3(256), 0, s, d_cols, d_pixels, channels_last, H, W, P, gh, gw, Kp,
                       0, groups, gpr);
  return hipGetLastError();
}

// ---- weight shadows: dst[Rp][Cp] = pad(cast(src[R][C])) and the transposed form dst[Cp][Rp] ------------
template <typename T>
__global__ __launch_bounds__(256) void cast_pad_kernel(const float* __restrict__ src, int R, int C, int ld,
                                                       T* __restrict__ dst, int Rp, int Cp, int ldd) {
  const size_t total = (size_t)Rp * Cp;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int c = (int)(idx % Cp);
    const int r = (int)(idx / Cp);
    const float v = (r < R && c < C) ? src[(size_t)r * ld + c] : 0.f;
    Elem<T>::st(dst + (size_t)r * ldd + c, v);
  }
}

hipError_t cast_pad(const float* src, int R, int C, int ld, void* dst, int dst_dtype, int Rp, int Cp, int ldd,
                    hipStream_t s) {
  const size_t total = (size_t)Rp * Cp;
  if (total == 0) return hipSuccess;
  int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  if (dst_dtype == DT_BF16)
    hipLaunchKernelGGL(cast_pad_kernel<bf16>, dim3(blocks), dim3(256), 0, s, src, R, C, ld, (bf16*)dst, Rp, Cp, ldd);
  else if (dst_dtype == DT_F16)
    hipLaunchKernelGGL(cast_pad_kernel<f16>, dim3(blocks), dim3(256), 0, s, src, R, C, ld, (f16*)dst, Rp, Cp, ldd);
  else
    hipLaunchKernelGGL(cast_pad_kernel<float>, dim3(blocks), dim3(256), 0, s, src, R, C, ld, (float*)dst, Rp, Cp, ldd);
  return hipGetLastError();
}

// ---- bf16x3 operand splits (compute mode SGL_DTYPE_BF16X3: strict arithmetic on the matrix cores) ------------------
// x = hi + lo + O(2^-17 |x|) with hi = bf16(x), lo = bf16(x - hi).  A product a*b is taken as hi*hi + hi*lo + lo*hi (the
// lo*lo term, 2^-18 relative, is dropped) by running ONE bf16 MFMA GEMM over a reduction dimension three times as long:
//   NT (reduction along the row):   A' row = [ hi | hi | lo ],  B' row = [ hi | lo | hi ]      (split3_rows)
//   TN (reduction down the rows):   A' = [ hi ; hi ; lo ],      B' = [ hi ; lo ; hi ]          (split3_stack)
// so the generation-6 kernels, their tile order and every fused epilogue are reused unchanged; accumulation is fp32.
__device__ __forceinline__ void split_bf16(float x, bf16& hi, bf16& lo) {
  hi = (bf16)x;
  lo = (bf16)(x - (float)hi);
}

// Row r of src (Cs = C rounded up to 8, zero filled) goes to dst + r * row_stride as hi, then at + seg_stride and
// + 2 * seg_stride as (hi, lo) for an A operand and (lo, hi) for a B operand (b_side).
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ src, int R, int C, int ld,
                                                     bf16* __restrict__ dst, int Cs, size_t row_stride, size_t seg_stride,
                                                     int b_side) {
  const int cpr = Cs >> 3;
  const size_t total = (size_t)R * cpr;
  const bool vec = ((ld & 3) == 0) && ((((uintptr_t)src) & 15) == 0);
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int r = (int)(idx / cpr), c0 = (int)(idx - (size_t)r * cpr) * 8;
    const float* sp = src + (size_t)r * ld + c0;
    float v[8];
    if (vec && c0 + 8 <= C) {
      Vec<float, 4>::ld(sp, v);
      Vec<float, 4>::ld(sp + 4, v + 4);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (c0 + j < C) ? sp[j] : 0.f;
    }
    bf16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bf16 h, l;
      split_bf16(v[j], h, l);
      hi[j] = h;
      lo[j] = l;
    }
    bf16* dp = dst + (size_t)r * row_stride + c0;
    *reinterpret_cast<bf16x8*>(dp) = hi;
    *reinterpret_cast<bf16x8*>(dp + seg_stride) = b_side ? lo : hi;
    *reinterpret_cast<bf16x8*>(dp + 2 * seg_stride) = b_side ? hi : lo;
  }
}

static hipError_t split3(const float* src, int R, int C, int ld, void* dst, int Cs, size_t row_stride, size_t seg_stride,
                         int b_side, hipStream_t s) {
  const size_t total = (size_t)R * (Cs / 8);
  if (total == 0) return hipSuccess;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(split3_kernel, dim3(blocks), dim3(256), 0, s, src, R, C, ld, (bf16*)dst, Cs, row_stride, seg_stride,
                     b_side);
  return hipGetLastError();
}
// dst [R][3*Cs] bf16: the three segments side by side in each row
hipError_t split3_rows(const float* src, int R, int C, int ld, void* dst, int Cs, int b_side, hipStream_t s) {
  return split3(src, R, C, ld, dst, Cs, 3 * (size_t)Cs, (size_t)Cs, b_side, s);
}
// dst [3*R][Cs] bf16: the three segments as planes of R rows, one below the other
hipError_t split3_stack(const float* src, int R, int C, int ld, void* dst, int Cs, int b_side, hipStream_t s) {
  return split3(src, R, C, ld, dst, Cs, (size_t)Cs, (size_t)R * Cs, b_side, s);
}

// ---- all weight shadows of one transformer block (or of the pooling head) in ONE launch -----------------------------------
// The per-step refresh of the compute-dtype weight copies (what autocast re-does every step in the reference,
// Siglip2sidafrozen.py:1375) used to be 13 launches per block (cast_pad + cast_transpose_pad per matrix, copy_f32 per bias):
// 350 launches of 5-7 us per so400m step, 153 per base-224 step.  Here a block's matrices are walked in 64x64 tiles of their
// PADDED destination (zeros outside the source), each tile read once as fp32 and written twice: row-major and, through an LDS
// transpose, column-major, both with >= 128-byte row segments; one extra workgroup copies / pads the bias vectors.
template <typename T>
__global__ __launch_bounds__(256) void cast_job_kernel(CastJob job) {
  __shared__ float lds_raw[64 * 66];
  T* lt = reinterpret_cast<T*>(lds_raw);
  const int t = threadIdx.x;
  int tile = blockIdx.x;
  if (tile >= job.ntiles) {   // the vectors: dst[i] = i < n ? src[i] : 0 for i < np  (fp32)
    for (int v = 0; v < job.nvec; ++v)
      for (int i = t; i < job.vnp[v]; i += 256) job.vdst[v][i] = (i < job.vn[v]) ? job.vsrc[v][i] : 0.f;
    return;
  }
  int mi = 0;
#pragma unroll
  for (int k = 1; k < 6; ++k) mi += (k < job.nmat && tile >= job.m[k].tile0) ? 1 : 0;
  CastMat m = job.m[0];
#pragma unroll
  for (int k = 1; k < 6; ++k)
    if (mi == k) m = job.m[k];
  tile -= m.tile0;
  const int tr = tile / m.tiles_c, tc = tile - tr * m.tiles_c;
  const int r0 = tr * 64, c0 = tc * 64;
  const int tx = t & 15, ty = t >> 4;
  // the padded destination [Rp][Cp] is written whole: zeros outside the R x C source
  const ShadowTile<T> sh{reinterpret_cast<T*>(m.dst), reinterpret_cast<T*>(m.dst_t), m.ldd, m.ldt, 0, m.Rp, m.Cp, 0, r0, c0, lt};
  const bool vsrc_ok = ((m.lds & 3) == 0) && ((((uintptr_t)m.src) & 15) == 0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 16 * k, cc = c0 + tx * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < m.R && cc < m.C) {
      const float* sp = m.src + (size_t)r * m.lds + cc;
      if (vsrc_ok && cc + 3 < m.C) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(sp);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
      } else {
        for (int j = 0; j < 4 && cc + j < m.C; ++j) v[j] = sp[j];
      }
    }
    sh.put(k, v);
  }
  sh.put_transposed();
}

void cast_job_add(CastJob& job, const float* src, int R, int C, int lds_, void* dst, int Rp, int Cp, int ldd, void* dst_t,
                  int ldt) {
  CastMat& m = job.m[job.nmat++];
  m.src = src; m.dst = dst; m.dst_t = dst_t;
  m.R = R; m.C = C; m.lds = lds_; m.Rp = Rp; m.Cp = Cp; m.ldd = ldd; m.ldt = ldt;
  m.tiles_c = (Cp + 63) / 64;
  m.tile0 = job.ntiles;
  job.ntiles += ((Rp + 63) / 64) * m.tiles_c;
}
void cast_job_add_vec(CastJob& job, const float* src, int n, float* dst, int np) {
  job.vsrc[job.nvec] = src; job.vdst[job.nvec] = dst; job.vn[job.nvec] = n; job.vnp[job.nvec] = np;
  ++job.nvec;
}
hipError_t cast_job_run(const CastJob& job, int dst_dtype, hipStream_t s) {
  if (job.ntiles == 0 && job.nvec == 0) return hipSuccess;
  const dim3 grid((unsigned)(job.ntiles + (job.nvec ? 1 : 0)));
  if (dst_dtype == DT_BF16)
    hipLaunchKernelGGL(cast_job_kernel<bf16>, grid, dim3(256), 0, s, job);
  else if (dst_dtype == DT_F16)
    hipLaunchKernelGGL(cast_job_kernel<f16>, grid, dim3(256), 0, s, job);
  else
    hipLaunchKernelGGL(cast_job_kernel<float>, grid, dim3(256), 0, s, job);
  return hipGetLastError();
}

// ---- column sums (bias gradients): two deterministic stages ------------------------------------------
int colsum_chunks(int M) {
  int c = (M + 511) / 512;
  return c < 1 ? 1 : (c > 256 ? 256 : c);
}

template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ in, int ld, int M, int N, int rows_per,
                                                     float* __restrict__ partial) {
  __shared__ float red[8][257];
  const int cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int col0 = blockIdx.x * 256 + cg * 8;
  const int r_begin = blockIdx.y * rows_per;
  const int r_end = (r_begin + rows_per < M) ? r_begin + rows_per : M;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (col0 < N) {
    for (int r = r_begin + rl; r < r_end; r += 8) {
      float v[8];
      Vec<T, 8>::ld(in + (size_t)r * ld + col0, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rl][cg * 8 + j] = acc[j];
  __syncthreads();
  const int c = threadIdx.x;
  if (blockIdx.x * 256 + c < N) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) s += red[r][c];
    partial[(size_t)blockIdx.y * N + blockIdx.x * 256 + c] = s;
  }
}

hipError_t colsum(const void* in, int dtype, int ld, int M, int N, int n_out, float* partial, float* out,
                  int accumulate, hipStream_t s) {
  if (N % 8 || ld % 8) return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  const int chunks = colsum_chunks(M);
  const int rows_per = (M + chunks - 1) / chunks;
  dim3 grid((N + 255) / 256, chunks), block(256);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(colsum_kernel<bf16>, grid, block, 0, s, (const bf16*)in, ld, M, N, rows_per, partial);
  else if (dtype == DT_F16)
    hipLaunchKernelGGL(colsum_kernel<f16>, grid, block, 0, s, (const f16*)in, ld, M, N, rows_per, partial);
  else
    hipLaunchKernelGGL(colsum_kernel<float>, grid, block, 0, s, (const float*)in, ld, M, N, rows_per, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return reduce_partials(partial, chunks, N, out, n_out < N ? n_out : N, accumulate, s);
}

// out[j] (+)= sum_b in[b*n + j]   (d pos-table = sum over images of d embeddings)
__global__ __launch_bounds__(256) void batch_sum_kernel(const float* __restrict__ in, int B, size_t n,
                                                        float* __restrict__ out, int accumulate) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += in[(size_t)b * n + j];
  out[j] = accumulate ? out[j] + s : s;
}
hipError_t batch_sum(const float* in, int B, size_t n, float* out, int accumulate, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(batch_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, B, n, out, accumulate);
  return hipGetLastError();
}

// out[j] (+)= sum_i v[i] * W[i*cols + j]: a row vector times a row-major fp32 matrix.  Block (x, y) sums row chunk y of 64
// columns (4 row groups folded through LDS) into partial[y][j]; reduce_partials folds the chunks in fixed order.
// Used for the v_proj bias gradient, see encoder.hip.  scratch: >= VECMAT_CHUNKS * cols floats.
constexpr int VECMAT_CHUNKS = 16;
__global__ __launch_bounds__(256) void vecmat_f32_kernel(const float* __restrict__ v, const float* __restrict__ W, int rows,
                                                         int cols, float* __restrict__ partial) {
  __shared__ float part[4][64];
  const int jj = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jj;
  const int per = (rows + VECMAT_CHUNKS - 1) / VECMAT_CHUNKS;
  const int r0 = blockIdx.y * per, r1 = (r0 + per < rows) ? r0 + per : rows;
  float s = 0.f;
  if (j < cols)
    for (int i = r0 + rg; i < r1; i += 4) s = fmaf(v[i], W[(size_t)i * cols + j], s);
  part[rg][jj] = s;
  __syncthreads();
  if (rg == 0 && j < cols) partial[(size_t)blockIdx.y * cols + j] = (part[0][jj] + part[1][jj]) + (part[2][jj] + part[3][jj]);
}
hipError_t vecmat_f32(const float* v, const float* W, int rows, int cols, float* scratch, float* out, int accumulate,
                      hipStream_t s) {
  if (rows <= 0 || cols <= 0) return hipSuccess;
  hipLaunchKernelGGL(vecmat_f32_kernel, dim3((unsigned)((cols + 63) / 64), VECMAT_CHUNKS), dim3(256), 0, s, v, W, rows, cols,
                     scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return reduce_partials(scratch, VECMAT_CHUNKS, cols, out, cols, accumulate, s);
}

// ---- position-table bicubic resize (F.interpolate bicubic, align_corners=False, A=-0.75;
//      TF:modeling_siglip.py:137-173).  Runs once per resolution; tiny. ---------------------------------
__device__ __forceinline__ void cubic_coeffs(float t, float* w) {
  const float A = -0.75f;
  float x = t + 1.0f;
  w[0] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
  x = t;
  w[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  x = 1.0f - t;
  w[2] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  x = 2.0f - t;
  w[3] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
}
__device__ __forceinline__ void cubic_taps(int o, int n_in, int n_out, int* idx, float* w) {
  const float scale = (float)n_in / (float)n_out;
  const float src = scale * ((float)o + 0.5f) - 0.5f;
  const float fl = floorf(src);
  cubic_coeffs(src - fl, w);
  const int i0 = (int)fl;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int i = i0 - 1 + k;
    idx[k] = i < 0 ? 0 : (i > n_in - 1 ? n_in - 1 : i);
  }
}

__global__ __launch_bounds__(256) void pos_resize_kernel(const float* __restrict__ table, int g0,
                                                         float* __restrict__ out, int gh, int gw, int D) {
  const size_t total = (size_t)gh * gw * D;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int d = (int)(idx % D);
  const int o = (int)(idx / D);
  const int oy = o / gw, ox = o - oy * gw;
  int iy[4], ix[4];
  float wy[4], wx[4];
  cubic_taps(oy, g0, gh, iy, wy);
  cubic_taps(ox, g0, gw, ix, wx);
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float rowv = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) rowv += wx[b] * table[((size_t)iy[a] * g0 + ix[b]) * D + d];
    acc += wy[a] * rowv;
  }
  out[idx] = acc;
}
hipError_t pos_resize(const float* table, int g0, float* out, int gh, int gw, int D, hipStream_t s) {
  const size_t total = (size_t)gh * gw * D;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(pos_resize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, table, g0, out, gh, gw,
                     D);
  return hipGetLastError();
}

// transpose of the above: dtable[iy][ix][d] (+)= sum over outputs (oy, ox) of wy(oy -> iy) * wx(ox -> ix) * dout[oy][ox][d].
// GATHER form, one thread per table element, contributions added in a fixed (oy, ox) order: bitwise reproducible (the
// round-1 scatter used 16 fp32 atomics per output element).  The outputs that can touch table row iy lie in a short range
// around (iy + 0.5) * gh / g0; it is scanned conservatively (+-3 source rows plus the border clamp) and the exact test is
// "one of the output's four clamped taps equals iy".
__device__ __forceinline__ void tap_range(int i, int g0, int gout, int& lo, int& hi) {
  const float inv = (float)gout / (float)g0;
  lo = (int)floorf(((float)i - 3.0f + 0.5f) * inv - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 3.0f + 0.5f) * inv - 0.5f) + 1;
  if (i == 0) lo = 0;                 // border entries also collect the clamped taps of every output near the edge
  if (i == g0 - 1) hi = gout - 1;
  if (lo < 0) lo = 0;
  if (hi > gout - 1) hi = gout - 1;
}
__global__ __launch_bounds__(256) void pos_resize_bwd_kernel(const float* __restrict__ dout, int gh, int gw,
                                                             float* __restrict__ dtable, int g0, int D) {
  const size_t total = (size_t)g0 * g0 * D;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int d = (int)(idx % D);
  const int e = (int)(idx / D);
  const int ty = e / g0, tx = e - ty * g0;
  int ylo, yhi, xlo, xhi;
  tap_range(ty, g0, gh, ylo, yhi);
  tap_range(tx, g0, gw, xlo, xhi);
  float acc = 0.f;
  for (int oy = ylo; oy <= yhi; ++oy) {
    int iy[4];
    float wy[4];
    cubic_taps(oy, g0, gh, iy, wy);
    float wyy = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) wyy += (iy[a] == ty) ? wy[a] : 0.f;
    if (wyy == 0.f) continue;
    float rowacc = 0.f;
    for (int ox = xlo; ox <= xhi; ++ox) {
      int ix[4];
      float wx[4];
      cubic_taps(ox, g0, gw, ix, wx);
      float wxx = 0.f;
#pragma unroll
      for (int b2 = 0; b2 < 4; ++b2) wxx += (ix[b2] == tx) ? wx[b2] : 0.f;
      if (wxx != 0.f) rowacc += wxx * dout[((size_t)oy * gw + ox) * D + d];
    }
    acc += wyy * rowacc;
  }
  dtable[idx] += acc;
}
hipError_t pos_resize_bwd(const float* dout, int gh, int gw, float* dtable, int g0, int D, hipStream_t s) {
  const size_t total = (size_t)g0 * g0 * D;
  if (total == 0 || gh * gw == 0) return hipSuccess;
  hipLaunchKernelGGL(pos_resize_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dout, gh, gw,
                     dtable, g0, D);
  return hipGetLastError();
}

// ---- small fp32 utilities ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void copy_f32_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ out, size_t n4, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<const f32x4*>(a)[i];
    if (b) v += reinterpret_cast<const f32x4*>(b)[i];
    reinterpret_cast<f32x4*>(out)[i] = v;
  }
  if (blockIdx.x == 0) {
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) out[i] = a[i] + (b ? b[i] : 0.f);
  }
}
hipError_t add_f32(const float* a, const float* b, float* out, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const size_t n4 = n / 4;
  size_t blocks = (n4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(copy_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, b, out, n4, n);
  return hipGetLastError();
}
hipError_t copy_f32(const float* src, float* dst, size_t n, hipStream_t s) { return add_f32(src, nullptr, dst, n, s); }

// dst[i] (+)= |0 * src[i]|: +0 where src[i] is finite, NaN where it is inf or NaN.  For a gradient that is zero in real
// arithmetic and is therefore never summed (the k_proj bias): it still has to turn non-finite when the pass it belongs to
// did, so that an overflowing step is seen in every gradient ("Non-finite values").
__global__ __launch_bounds__(256) void zero_unless_nonfinite_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                    int n, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float z = fabsf(src[i] * 0.f);
  dst[i] = accumulate ? dst[i] + z : z;
}
hipError_t zero_unless_nonfinite(const float* src, float* dst, int n, int accumulate, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(zero_unless_nonfinite_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n,
                     accumulate);
  return hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(256) void cast_f32_kernel(const float* __restrict__ a, T* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    Elem<T>::st(out + i, a[i]);
}
hipError_t cast_f32(const float* src, void* dst, int dst_dtype, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (dst_dtype == DT_BF16)
    hipLaunchKernelGGL(cast_f32_kernel<bf16>, dim3((unsigned)blocks), dim3(256), 0, s, src, (bf16*)dst, n);
  else if (dst_dtype == DT_F16)
    hipLaunchKernelGGL(cast_f32_kernel<f16>, dim3((unsigned)blocks), dim3(256), 0, s, src, (f16*)dst, n);
  else
    hipLaunchKernelGGL(cast_f32_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, src, (float*)dst, n);
  return hipGetLastError();
}

// ---- split-K slabs -> result, fixed order -----------------------------------------------------------------
__global__ __launch_bounds__(256) void reduce_splits_kernel(const float* __restrict__ ws, int splits, size_t stride,
                                                            int N1, int N2, float* __restrict__ out, int ldo,
                                                            int accumulate) {
  const size_t total4 = ((size_t)N1 * N2) >> 2;  // N2 % 4 == 0 (checked by the host)
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
    const size_t e = i << 2;
    const int r = (int)(e / N2), c = (int)(e - (size_t)r * N2);
    f32x4 a = *reinterpret_cast<const f32x4*>(ws + e);
    for (int s = 1; s < splits; ++s) a += *reinterpret_cast<const f32x4*>(ws + (size_t)s * stride + e);
    float* o = out + (size_t)r * ldo + c;
    if (accumulate) a += *reinterpret_cast<const f32x4*>(o);
    *reinterpret_cast<f32x4*>(o) = a;
  }
}

hipError_t reduce_splits(const float* ws, int splits, size_t stride, int N1, int N2, float* out, int ldo, int accumulate,
                         hipStream_t s) {
  if ((N2 & 3) || (ldo & 3) || (((uintptr_t)out) & 15) || (((uintptr_t)ws) & 15) || (stride & 3))
    return hipErrorInvalidValue;
  const size_t total4 = ((size_t)N1 * N2) >> 2;
  if (total4 == 0) return hipSuccess;
  const int blocks = (int)((total4 + 255) / 256 < 2048 ? (total4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(reduce_splits_kernel, dim3(blocks), dim3(256), 0, s, ws, splits, stride, N1, N2, out, ldo,
                     accumulate);
  return hipGetLastError();
}

}  // namespace sgl
