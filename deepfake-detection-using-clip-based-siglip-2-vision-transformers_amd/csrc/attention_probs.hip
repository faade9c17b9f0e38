// Attention probabilities of one block, recomputed from what a saving forward keeps: the head-major q, k and the row
// log-sum-exp.  p[b,h,i,j] = exp2(S_ij * c - lse_i * log2e), S = q·kᵀ, c = log2e / sqrt(dh): the same expression, on the
// same operands and constants, as the P the two backward kernels of attention.hip rebuild.  lse is used as given (rows are
// not renormalised), every input is const, nothing but `out` is written.
//   FULL       out (B,H,N,N) fp32
//   HEAD_MEAN  out (B,N,N)   fp32 = (sum_h p[b,h]) / H   (heads summed in ascending order in registers, one division by
//              H, one store: the per-head maps never exist in memory.  The division is IEEE, so the H - 1 additions and
//              it keep the result within H * 2^-24 of the exact mean; a multiply by a rounded 1/H would cost two
//              roundings whenever H is not a power of two)
// No atomics, no LDS, no barriers; each output element is written by exactly one 4-byte store, so a call is bitwise
// reproducible.  Rows / keys >= N are never stored (their operand fragments read as zeros through the buffer bounds check).
//
// 16-bit kernel: a workgroup of 4 waves owns a 128 x 128 tile of one image (HEAD_MEAN) or of one (image, head) (FULL); wave
// w owns query rows 32w .. 32w+31 and the four 32-key sub-tiles.  S = Q·Kᵀ on v_mfma_f32_32x32x16_{bf16,f16} with A = Q
// and B = K, both fragments 16 bytes per lane straight from global memory (row = lane & 31, columns 8 * (lane >> 5) .. + 7
// of the k-step: the operand layout the backward's kfr / vfr loads use).  The C tile then has the KEY on the lane:
// register i of lane l is query row 8 * (i >> 2) + 4 * (l >> 5) + (i & 3), key l & 31, so one store instruction writes two
// contiguous 128-byte row segments.  Output rows are N floats: nothing wider than 4 bytes is aligned for odd N.
// fp32 operands take the routes of the matching forward kernels: v_mfma_f32_32x32x2_f32 with the k-steps in the order of
// attention_f32.hip (SGL_DTYPE_BF16X3), or one fp32 FMA chain over d = 0 .. dh-1 per score as attention_ref.hip (F32);
// both then form expf(S * scale - lse) as those kernels' backward passes do.  Neither is a performance path.
#include "common.hip.h"
#include "kernels.h"

namespace sgl {

namespace {

constexpr float AP_LOG2E = 1.4426950408889634f;

// workgroup -> (z, query tile, key tile), key tile fastest: the workgroups of one query tile share its Q rows in L2
__device__ __forceinline__ void ap_tile(int nqt, int nkt, int& z, int& qt, int& kt) {
  unsigned pid = blockIdx.x;
  kt = (int)(pid % (unsigned)nkt);
  pid /= (unsigned)nkt;
  qt = (int)(pid % (unsigned)nqt);
  z = (int)(pid / (unsigned)nqt);
}

// store C-tile registers: row0 + row(i, hh), column `col` (both already known to be < N where stored)
__device__ __forceinline__ void ap_store(float* __restrict__ out, size_t zbase, const f32x16& p, int row0, int hh, int col,
                                         int N) {
  if (col >= N) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = row0 + 8 * (i >> 2) + 4 * hh + (i & 3);
    if (row < N) out[zbase + (size_t)row * (size_t)N + (size_t)col] = p[i];
  }
}

template <typename T, int DP, bool MEAN>
__global__ __launch_bounds__(256) void attn_probs_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                         const float* __restrict__ lse, float* __restrict__ out, int H,
                                                         int N, int nqt, int nkt, float c, float heads) {
  constexpr int KS = DP / 16;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, hh = lane >> 5;
  int z, qt, kt;
  ap_tile(nqt, nkt, z, qt, kt);
  const int q0 = qt * 128 + w * 32, k0 = kt * 128;
  if (q0 >= N) return;   // wave-uniform; the kernel has no barrier
  const int nh = MEAN ? H : 1;
  const uint32_t hbytes = (uint32_t)((size_t)N * DP * 2);
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  const size_t zbase = (size_t)z * (size_t)N * (size_t)N;

  for (int hd = 0; hd < nh; ++hd) {
    const size_t bh = MEAN ? (size_t)z * H + hd : (size_t)z;
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(Q + bh * (size_t)N * DP, hbytes);
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(K + bh * (size_t)N * DP, hbytes);
    lo_x8<T> qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      qf[ks] = __builtin_bit_cast(
          lo_x8<T>, __builtin_amdgcn_raw_buffer_load_b128(
                        rq, (q0 + li < N) ? (uint32_t)(q0 + li) * (uint32_t)(DP * 2) + (uint32_t)(2 * ks + hh) * 16u : SGL_OOB,
                        0, 0));
    float L[16];   // -lse * log2e of this lane's 16 query rows, the addend of the backward kernels' fused multiply-add
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = q0 + 8 * (i >> 2) + 4 * hh + (i & 3);
      L[i] = (row < N) ? -lse[bh * (size_t)N + row] * AP_LOG2E : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kb = k0 + 32 * j;
      if (kb < N) {   // wave-uniform
        lo_x8<T> kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          kf[ks] = __builtin_bit_cast(
              lo_x8<T>,
              __builtin_amdgcn_raw_buffer_load_b128(
                  rk, (kb + li < N) ? (uint32_t)(kb + li) * (uint32_t)(DP * 2) + (uint32_t)(2 * ks + hh) * 16u : SGL_OOB, 0, 0));
        f32x16 S;
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) S = mfma_32x32x16(qf[ks], kf[ks], S);
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i] = __builtin_amdgcn_exp2f(fmaf(S[i], c, L[i]));
        if constexpr (MEAN) {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[j][i] += S[i];
        } else {
          ap_store(out, zbase, S, q0, hh, kb + li, N);
        }
      }
    }
  }
  if constexpr (MEAN) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kb = k0 + 32 * j;
      if (kb < N) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] /= heads;
        ap_store(out, zbase, acc[j], q0, hh, kb + li, N);
      }
    }
  }
}

// fp32 operands on v_mfma_f32_32x32x2_f32: A[m][k] from lane (m = lane & 31, k = lane >> 5), B[k][n] likewise; k-steps in
// ascending order as attention_f32.hip.  Same tile ownership and C layout as the 16-bit kernel.
template <bool MEAN>
__global__ __launch_bounds__(256) void attn_probs_f32_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                             const float* __restrict__ lse, float* __restrict__ out,
                                                             int H, int N, int dh, int DP, int nqt, int nkt, float scale,
                                                             float heads) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, hh = lane >> 5;
  int z, qt, kt;
  ap_tile(nqt, nkt, z, qt, kt);
  const int q0 = qt * 128 + w * 32, k0 = kt * 128;
  if (q0 >= N) return;
  const int nh = MEAN ? H : 1;
  const int ks = dh / 2;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  const size_t zbase = (size_t)z * (size_t)N * (size_t)N;
  const bool qok = q0 + li < N;

  for (int hd = 0; hd < nh; ++hd) {
    const size_t bh = MEAN ? (size_t)z * H + hd : (size_t)z;
    const float* qrow = Q + bh * (size_t)N * DP + (size_t)(qok ? q0 + li : 0) * DP + hh;
    float L[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = q0 + 8 * (i >> 2) + 4 * hh + (i & 3);
      L[i] = (row < N) ? lse[bh * (size_t)N + row] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kb = k0 + 32 * j;
      if (kb < N) {
        const bool kok = kb + li < N;
        const float* krow = K + bh * (size_t)N * DP + (size_t)(kok ? kb + li : 0) * DP + hh;
        f32x16 S;
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i] = 0.f;
        for (int s = 0; s < ks; ++s) {
          const float a = qok ? qrow[2 * s] : 0.f;
          const float b = kok ? krow[2 * s] : 0.f;
          S = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, S, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i] = expf(S[i] * scale - L[i]);
        if constexpr (MEAN) {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[j][i] += S[i];
        } else {
          ap_store(out, zbase, S, q0, hh, kb + li, N);
        }
      }
    }
  }
  if constexpr (MEAN) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kb = k0 + 32 * j;
      if (kb < N) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] /= heads;
        ap_store(out, zbase, acc[j], q0, hh, kb + li, N);
      }
    }
  }
}

// strict fp32: one thread per output element (key on the lane, 4 query rows per workgroup), one FMA chain per score
template <bool MEAN>
__global__ __launch_bounds__(256) void attn_probs_ref_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                             const float* __restrict__ lse, float* __restrict__ out,
                                                             int H, int N, int dh, int DP, int nqt, int nkt, float scale,
                                                             float heads) {
  int z, qt, kt;
  ap_tile(nqt, nkt, z, qt, kt);
  const int row = qt * 4 + (int)(threadIdx.x >> 6), col = kt * 64 + (int)(threadIdx.x & 63);
  if (row >= N || col >= N) return;
  const int nh = MEAN ? H : 1;
  float acc = 0.f;
  for (int hd = 0; hd < nh; ++hd) {
    const size_t bh = MEAN ? (size_t)z * H + hd : (size_t)z;
    const float* qr = Q + (bh * (size_t)N + row) * DP;
    const float* kr = K + (bh * (size_t)N + col) * DP;
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s = fmaf(qr[d], kr[d], s);
    acc += expf(s * scale - lse[bh * (size_t)N + row]);
  }
  if constexpr (MEAN) acc /= heads;
  out[(size_t)z * (size_t)N * (size_t)N + (size_t)row * (size_t)N + (size_t)col] = acc;
}

// pooling head: probs [B][H][N] -> out [B][N] = (sum_h probs[b,h,n]) / H, heads in ascending order
__global__ __launch_bounds__(256) void head_mean_kernel(const float* __restrict__ probs, float* __restrict__ out, int H,
                                                        int N, size_t total, float heads) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t b = idx / (size_t)N, n = idx - b * (size_t)N;
  float acc = 0.f;
  for (int h = 0; h < H; ++h) acc += probs[(b * H + h) * (size_t)N + n];
  out[idx] = acc / heads;
}

template <typename T, int DP>
hipError_t ap_launch(const void* q, const void* k, const float* lse, float* out, int B, int H, int N, int dh, int mode,
                     hipStream_t s) {
  const int nt = (N + 127) / 128;
  const float c = (1.0f / sqrtf((float)dh)) * AP_LOG2E;
  const unsigned grid = (unsigned)((size_t)nt * nt * (mode ? B : B * H));
  if (mode)
    hipLaunchKernelGGL((attn_probs_kernel<T, DP, true>), dim3(grid), dim3(256), 0, s, (const T*)q, (const T*)k, lse, out, H,
                       N, nt, nt, c, (float)H);
  else
    hipLaunchKernelGGL((attn_probs_kernel<T, DP, false>), dim3(grid), dim3(256), 0, s, (const T*)q, (const T*)k, lse, out, H,
                       N, nt, nt, c, 1.0f);
  return hipGetLastError();
}

}  // namespace

bool attn_probs_shape_ok(int dtype, int B, int H, int N, int dh, int DP) {
  if (B < 1 || H < 1 || N < 1 || dh < 1 || dh > DP) return false;
  size_t wgs;   // workgroups of the FULL launch (the larger one): a 1-D grid
  if (dtype == DT_F32) {
    if (dh > 128) return false;
    wgs = (size_t)((N + 3) / 4) * ((N + 63) / 64);
  } else {
    if (dtype == DT_F32_MFMA) {
      if (dh % 8 || dh > 96 || DP % 4) return false;
    } else {
      if (dh % 8 || DP != ((dh + 15) / 16) * 16 || DP > 96) return false;
      if ((size_t)N * DP * 2 >= (1ull << 31)) return false;
    }
    wgs = (size_t)((N + 127) / 128) * ((N + 127) / 128);
  }
  return wgs * (size_t)B * (size_t)H < (1ull << 31);
}

hipError_t probs_head_mean(const float* probs, float* out, int B, int H, int N, hipStream_t s) {
  const size_t total = (size_t)B * N;
  if (B < 1 || H < 1 || N < 1 || (total + 255) / 256 >= (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(head_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, probs, out, H, N, total,
                     (float)H);
  return hipGetLastError();
}

hipError_t attn_probs(const void* q, const void* k, const float* lse, float* out, int dtype, int B, int H, int N, int dh,
                      int DP, int mode, hipStream_t s) {
  if (mode != SGL_ATTN_PROBS_FULL && mode != SGL_ATTN_PROBS_HEAD_MEAN) return hipErrorInvalidValue;
  if (!attn_probs_shape_ok(dtype, B, H, N, dh, DP)) return hipErrorInvalidValue;
  const int Z = mode ? B : B * H;
  const float scale = 1.0f / sqrtf((float)dh), heads = (float)H;
  if (dtype == DT_F32 || dtype == DT_F32_MFMA) {
    const float* qf = (const float*)q;
    const float* kf = (const float*)k;
    if (dtype == DT_F32) {
      const int nqt = (N + 3) / 4, nkt = (N + 63) / 64;
      const dim3 grid((unsigned)((size_t)nqt * nkt * Z));
      if (mode)
        hipLaunchKernelGGL(attn_probs_ref_kernel<true>, grid, dim3(256), 0, s, qf, kf, lse, out, H, N, dh, DP, nqt, nkt, scale,
                           heads);
      else
        hipLaunchKernelGGL(attn_probs_ref_kernel<false>, grid, dim3(256), 0, s, qf, kf, lse, out, H, N, dh, DP, nqt, nkt,
                           scale, heads);
    } else {
      const int nt = (N + 127) / 128;
      const dim3 grid((unsigned)((size_t)nt * nt * Z));
      if (mode)
        hipLaunchKernelGGL(attn_probs_f32_kernel<true>, grid, dim3(256), 0, s, qf, kf, lse, out, H, N, dh, DP, nt, nt, scale,
                           heads);
      else
        hipLaunchKernelGGL(attn_probs_f32_kernel<false>, grid, dim3(256), 0, s, qf, kf, lse, out, H, N, dh, DP, nt, nt, scale,
                           heads);
    }
    return hipGetLastError();
  }
  if (dtype != DT_BF16 && dtype != DT_F16) return hipErrorInvalidValue;
  if ((((uintptr_t)q) | ((uintptr_t)k)) & 15) return hipErrorInvalidValue;
#define SGL_P(T, DPV) \
  case DPV: return ap_launch<T, DPV>(q, k, lse, out, B, H, N, dh, mode, s);
  if (dtype == DT_F16) {
    switch (DP) { SGL_P(f16, 16) SGL_P(f16, 32) SGL_P(f16, 48) SGL_P(f16, 64) SGL_P(f16, 80) SGL_P(f16, 96) }
    return hipErrorInvalidValue;
  }
  switch (DP) { SGL_P(bf16, 16) SGL_P(bf16, 32) SGL_P(bf16, 48) SGL_P(bf16, 64) SGL_P(bf16, 80) SGL_P(bf16, 96) }
#undef SGL_P
  return hipErrorInvalidValue;
}

}  // namespace sgl
