// The attention-pooling head's kernels (sgl_op_pool_attn_fwd / _bwd and the encoder's head stage).
#include "attention.hip.h"
#include "common.hip.h"
#include "kernels.h"

namespace sgl {

// launch(T{}) for the K/V element type of `dtype`: bf16, f16 or (anything else) float
template <typename Launch>
static hipError_t pool_dispatch(int dtype, Launch&& launch) {
  if (dtype == DT_BF16) launch(bf16{});
  else if (dtype == DT_F16) launch(f16{});
  else launch(float{});
  return hipGetLastError();
}

// ---- attention-pool head: one probe query per image (TF:modeling_siglip.py:633-637, nn.MultiheadAttention
//      with q = probe, k = v = tokens).  One block per (b, h).  < 0.1 % of the FLOPs, HBM-bound: K and V of the
//      head are read once, in 16-byte (bf16) / 32-byte (fp32) chunks with consecutive lanes on consecutive chunks.
//      Thread t of the first RP*CPR (RP = 256 / CPR rows per pass, CPR = DP/8 chunks per row) owns chunk column
//      t % CPR for rows t / CPR, + RP, + 2 RP, ...: its slice of q / dO stays in registers. ---------------------
template <typename T>
__device__ __forceinline__ float block_reduce_256(float v, float* red, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T>
__global__ __launch_bounds__(256) void pool_attn_fwd_kernel(const float* __restrict__ q, const T* __restrict__ K,
                                                            const T* __restrict__ V, T* __restrict__ out,
                                                            float* __restrict__ probs, int H, int N, int dh, int DP) {
  extern __shared__ __attribute__((aligned(16))) float pa_smem[];  // [N*CPR] chunk partials, [N] probabilities, [8] scratch
  const int CPR = DP >> 3, RP = 256 / CPR;
  float* part = pa_smem;
  float* pr = part + (size_t)N * CPR;
  float* red = pr + N;
  const int bh = blockIdx.x, h = bh % H, b = bh / H;
  const T* Kb = K + (size_t)bh * N * DP;
  const T* Vb = V + (size_t)bh * N * DP;
  const float scale = rsqrtf((float)dh);
  const int t = threadIdx.x, c = t % CPR, r0 = t / CPR;
  const bool act = t < RP * CPR;
  float qv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) qv[j] = (c * 8 + j < dh) ? q[h * dh + c * 8 + j] : 0.f;
  if (act)
    for (int n = r0; n < N; n += RP) {
      float kv[8];
      Vec<T, 8>::ld(Kb + (size_t)n * DP + c * 8, kv);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s = fmaf(qv[j], kv[j], s);
      part[n * CPR + c] = s;
    }
  __syncthreads();
  float mx = -INFINITY;
  for (int n = t; n < N; n += 256) {
    float s = 0.f;
    for (int j = 0; j < CPR; ++j) s += part[n * CPR + j];
    s *= scale;
    pr[n] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_reduce_256<T>(mx, red, true);
  float sum = 0.f;
  for (int n = t; n < N; n += 256) {
    const float e = __expf(pr[n] - mx);
    pr[n] = e;
    sum += e;
  }
  sum = block_reduce_256<T>(sum, red, false);
  const float inv = 1.0f / sum;
  for (int n = t; n < N; n += 256) {
    const float pv = pr[n] * inv;
    pr[n] = pv;
    probs[(size_t)bh * N + n] = pv;
  }
  __syncthreads();
  // out[d] = sum_n p_n V[n, d]: per-thread partial over its rows, then the RP threads of a chunk column through LDS
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (act)
    for (int n = r0; n < N; n += RP) {
      float vv[8];
      Vec<T, 8>::ld(Vb + (size_t)n * DP + c * 8, vv);
      const float pv = pr[n];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(pv, vv[j], acc[j]);
    }
  __syncthreads();   // part[] is free again
  if (act) {
#pragma unroll
    for (int j = 0; j < 8; ++j) part[(r0 * CPR + c) * 8 + j] = acc[j];
  }
  __syncthreads();
  for (int d = t; d < dh; d += 256) {
    float a = 0.f;
    for (int r = 0; r < RP; ++r) a += part[(r * CPR + (d >> 3)) * 8 + (d & 7)];
    Elem<T>::st(out + (size_t)b * H * dh + h * dh + d, a);
  }
}

hipError_t pool_attn_fwd(const float* q, const void* K, const void* V, int dtype, void* out, float* probs, int B,
                         int H, int N, int dh, int DP, hipStream_t s) {
  if (B * H == 0) return hipSuccess;
  if (DP % 8 || DP < 8 || DP > 2048) return hipErrorInvalidValue;
  if (N < 0 || N > pool_attn_max_tokens(DP, 0)) return hipErrorInvalidValue;   // the default LDS window (kernels.h)
  const size_t smem = pool_attn_lds_floats(N, DP, 0) * sizeof(float);
  return pool_dispatch(dtype, [&](auto elem) {
    using T = decltype(elem);
    hipLaunchKernelGGL(pool_attn_fwd_kernel<T>, dim3(B * H), dim3(256), smem, s, q, (const T*)K, (const T*)V, (T*)out,
                       probs, H, N, dh, DP);
  });
}

// Ragged batch: pool_attn_fwd_kernel on segment `seg` of a packed batch.  K, V head-major [H][T][DP]; one block per
// (segment, head) works on the segment's N rows from its first row (seg_range's clamp, attention.hip.h), with the same
// per-thread row walk and the same reduction order, so a segment gets the bits pool_attn_fwd_kernel gives an image of N
// tokens.  The LDS window is sized for max_n.  out [S][H*dh], probs [H][T].
template <typename T>
__global__ __launch_bounds__(256) void pool_attn_fwd_varlen_kernel(const float* __restrict__ q, const T* __restrict__ K,
                                                                   const T* __restrict__ V, T* __restrict__ out,
                                                                   float* __restrict__ probs, const int* __restrict__ cu,
                                                                   int Ttot, int max_n, int H, int dh, int DP) {
  extern __shared__ __attribute__((aligned(16))) float pa_smem[];  // [N*CPR] chunk partials, [N] probabilities, [8] scratch
  const int CPR = DP >> 3, RP = 256 / CPR;
  const int bh = blockIdx.x, h = bh % H, b = bh / H;
  int row0, N;
  seg_range(cu, b, Ttot, max_n, row0, N);
  float* part = pa_smem;
  float* pr = part + (size_t)N * CPR;
  float* red = pr + N;
  const T* Kb = K + ((size_t)h * Ttot + row0) * DP;
  const T* Vb = V + ((size_t)h * Ttot + row0) * DP;
  float* prow = probs + (size_t)h * Ttot + row0;
  const float scale = rsqrtf((float)dh);
  const int t = threadIdx.x, c = t % CPR, r0 = t / CPR;
  const bool act = t < RP * CPR;
  float qv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) qv[j] = (c * 8 + j < dh) ? q[h * dh + c * 8 + j] : 0.f;
  if (act)
    for (int n = r0; n < N; n += RP) {
      float kv[8];
      Vec<T, 8>::ld(Kb + (size_t)n * DP + c * 8, kv);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s = fmaf(qv[j], kv[j], s);
      part[n * CPR + c] = s;
    }
  __syncthreads();
  float mx = -INFINITY;
  for (int n = t; n < N; n += 256) {
    float s = 0.f;
    for (int j = 0; j < CPR; ++j) s += part[n * CPR + j];
    s *= scale;
    pr[n] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_reduce_256<T>(mx, red, true);
  float sum = 0.f;
  for (int n = t; n < N; n += 256) {
    const float e = __expf(pr[n] - mx);
    pr[n] = e;
    sum += e;
  }
  sum = block_reduce_256<T>(sum, red, false);
  const float inv = 1.0f / sum;
  for (int n = t; n < N; n += 256) {
    const float pv = pr[n] * inv;
    pr[n] = pv;
    prow[n] = pv;
  }
  __syncthreads();
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (act)
    for (int n = r0; n < N; n += RP) {
      float vv[8];
      Vec<T, 8>::ld(Vb + (size_t)n * DP + c * 8, vv);
      const float pv = pr[n];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(pv, vv[j], acc[j]);
    }
  __syncthreads();   // part[] is free again
  if (act) {
#pragma unroll
    for (int j = 0; j < 8; ++j) part[(r0 * CPR + c) * 8 + j] = acc[j];
  }
  __syncthreads();
  for (int d = t; d < dh; d += 256) {
    float a = 0.f;
    for (int r = 0; r < RP; ++r) a += part[(r * CPR + (d >> 3)) * 8 + (d & 7)];
    Elem<T>::st(out + (size_t)b * H * dh + h * dh + d, a);
  }
}

hipError_t pool_attn_fwd_varlen(const float* q, const void* K, const void* V, int dtype, void* out, float* probs,
                                const int* cu, int S, int T, int max_n, int H, int dh, int DP, hipStream_t s) {
  if (S < 1 || H < 1 || T < 1 || (size_t)S * H >= (1ull << 31)) return hipErrorInvalidValue;
  if (DP % 8 || DP < 8 || DP > 2048) return hipErrorInvalidValue;
  if (max_n < 1 || max_n > pool_attn_max_tokens(DP, 0)) return hipErrorInvalidValue;   // the default LDS window (kernels.h)
  const size_t smem = pool_attn_lds_floats(max_n, DP, 0) * sizeof(float);
  return pool_dispatch(dtype, [&](auto elem) {
    using E = decltype(elem);
    hipLaunchKernelGGL(pool_attn_fwd_varlen_kernel<E>, dim3(S * H), dim3(256), smem, s, q, (const E*)K, (const E*)V,
                       (E*)out, probs, cu, T, max_n, H, dh, DP);
  });
}

// The device table of a ragged batch from host lengths: cu[i] = lens[0] + ... + lens[i-1], i = 0 .. S.  The prefix sums
// are formed on the host and travel BY VALUE in the kernel arguments, 256 per launch (as sgl_op_preprocess_views moves its
// records): no copy from host memory, no allocation, no synchronisation, the caller's stream only; plain vector stores.
constexpr int kSegChunk = 256;
struct SegChunk {
  int v[kSegChunk];
};
__global__ __launch_bounds__(kSegChunk) void seg_offsets_kernel(SegChunk chunk, int n, int* __restrict__ cu) {
  const int i = threadIdx.x;
  if (i < n) cu[i] = chunk.v[i];
}

hipError_t seg_offsets(const int* lens, int S, int* cu, hipStream_t s) {
  static_assert(sizeof(SegChunk) <= 2048, "a chunk of offsets must fit the kernel arguments");
  if (S < 1) return hipErrorInvalidValue;
  long long total = 0;
  for (int i = 0; i < S; ++i) {
    if (lens[i] < 0) return hipErrorInvalidValue;
    total += lens[i];
  }
  if (total > 0x7fffffffLL) return hipErrorInvalidValue;
  int run = 0;
  for (int i0 = 0; i0 <= S; i0 += kSegChunk) {
    const int n = S + 1 - i0 < kSegChunk ? S + 1 - i0 : kSegChunk;
    SegChunk chunk = {};
    for (int i = 0; i < n; ++i) {
      chunk.v[i] = run;
      if (i0 + i < S) run += lens[i0 + i];
    }
    hipLaunchKernelGGL(seg_offsets_kernel, dim3(1), dim3(kSegChunk), 0, s, chunk, n, cu + i0);
  }
  return hipGetLastError();
}

// backward: dV[n,d] = p_n * do[d];  dp_n = do·V[n];  ds_n = p_n (dp_n - Σ p dp) * scale;
//           dK[n,d] = ds_n q[d];   dq[d] (per image) = Σ_n ds_n K[n,d]
// dkv is token-major [B*N][2*H*dh] (k block then v block) — the A operand of the kv-projection backward GEMMs.
template <typename T>
__global__ __launch_bounds__(256) void pool_attn_bwd_kernel(const float* __restrict__ q, const T* __restrict__ K,
                                                            const T* __restrict__ V, const float* __restrict__ probs,
                                                            const float* __restrict__ dout, T* __restrict__ dkv,
                                                            float* __restrict__ dq_partial, int H, int N, int dh,
                                                            int DP) {
  extern __shared__ __attribute__((aligned(16))) float pa_smem[];  // [N*CPR] chunk partials, [N] ds, [N] p, [8] scratch
  const int CPR = DP >> 3, RP = 256 / CPR;
  float* part = pa_smem;
  float* ds = part + (size_t)N * CPR;
  float* pr = ds + N;
  float* red = pr + N;
  const int bh = blockIdx.x, h = bh % H, b = bh / H;
  const int D = H * dh;
  const T* Kb = K + (size_t)bh * N * DP;
  const T* Vb = V + (size_t)bh * N * DP;
  const float scale = rsqrtf((float)dh);
  const int t = threadIdx.x, c = t % CPR, r0 = t / CPR;
  const bool act = t < RP * CPR;
  const bool real = c * 8 < dh;     // dh % 8 == 0: a chunk is entirely data or entirely pad
  float qv[8], dov[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    qv[j] = real ? q[h * dh + c * 8 + j] : 0.f;
    dov[j] = real ? dout[(size_t)b * D + h * dh + c * 8 + j] : 0.f;
  }
  if (act)
    for (int n = r0; n < N; n += RP) {
      float vv[8];
      Vec<T, 8>::ld(Vb + (size_t)n * DP + c * 8, vv);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s = fmaf(dov[j], vv[j], s);
      part[n * CPR + c] = s;
    }
  __syncthreads();
  float psum = 0.f;
  for (int n = t; n < N; n += 256) {
    float dp = 0.f;
    for (int j = 0; j < CPR; ++j) dp += part[n * CPR + j];
    const float pv = probs[(size_t)bh * N + n];
    ds[n] = dp;
    pr[n] = pv;
    psum += pv * dp;
  }
  const float dot = block_reduce_256<T>(psum, red, false);
  for (int n = t; n < N; n += 256) ds[n] = pr[n] * (ds[n] - dot) * scale;
  __syncthreads();
  // dK / dV rows (16-byte chunks, 9 consecutive lanes per 144-byte row segment) and the per-thread part of dq
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (act)
    for (int n = r0; n < N; n += RP) {
      float kv[8];
      Vec<T, 8>::ld(Kb + (size_t)n * DP + c * 8, kv);
      const float g = ds[n], pv = pr[n];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(g, kv[j], acc[j]);
      if (real) {
        float ok[8], ov[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          ok[j] = g * qv[j];
          ov[j] = pv * dov[j];
        }
        T* row = dkv + ((size_t)b * N + n) * (2 * (size_t)D) + h * dh + c * 8;
        Vec<T, 8>::st(row, ok);
        Vec<T, 8>::st(row + D, ov);
      }
    }
  __syncthreads();   // part[] is free again
  if (act) {
#pragma unroll
    for (int j = 0; j < 8; ++j) part[(r0 * CPR + c) * 8 + j] = acc[j];
  }
  __syncthreads();
  for (int d = t; d < dh; d += 256) {
    float a = 0.f;
    for (int r = 0; r < RP; ++r) a += part[(r * CPR + (d >> 3)) * 8 + (d & 7)];
    dq_partial[(size_t)b * D + h * dh + d] = a;
  }
}

hipError_t pool_attn_bwd(const float* q, const void* K, const void* V, int dtype, const float* probs,
                         const float* dout, void* dkv, float* dq_partial, int B, int H, int N, int dh, int DP,
                         hipStream_t s) {
  if (B * H == 0) return hipSuccess;
  if (DP % 8 || dh % 8 || DP < 8 || DP > 2048) return hipErrorInvalidValue;
  if (N < 0 || N > pool_attn_max_tokens(DP, 1)) return hipErrorInvalidValue;   // the default LDS window (kernels.h)
  const size_t smem = pool_attn_lds_floats(N, DP, 1) * sizeof(float);
  return pool_dispatch(dtype, [&](auto elem) {
    using T = decltype(elem);
    hipLaunchKernelGGL(pool_attn_bwd_kernel<T>, dim3(B * H), dim3(256), smem, s, q, (const T*)K, (const T*)V, probs, dout,
                       (T*)dkv, dq_partial, H, N, dh, DP);
  });
}

// The probe row's counterpart of attention_grad_probs.hip: da[b,h,n] = sum_d dout[b,h*dh+d] * V[b,h,n,d] (one FMA chain,
// d ascending, over the dh real columns: V's pad is never read), combined with the probabilities the forward kept.
// One thread per output element; MEAN sums the heads in ascending order and divides once.  Plain stores, inputs const.
template <typename T, bool MEAN>
__global__ __launch_bounds__(256) void pool_attn_grad_probs_kernel(const T* __restrict__ V, const float* __restrict__ probs,
                                                                   const float* __restrict__ dout,
                                                                   float* __restrict__ out, int H, int N, int dh, int DP,
                                                                   size_t total, float heads, int kind) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t n = idx % (size_t)N, z = idx / (size_t)N;
  const int nh = MEAN ? H : 1;
  float acc = 0.f;
  for (int hd = 0; hd < nh; ++hd) {
    const size_t bh = MEAN ? z * H + hd : z;
    const float* go = dout + bh * (size_t)dh;   // [B][H*dh]: head (b, h) starts at (b*H + h) * dh
    const T* vr = V + (bh * (size_t)N + n) * (size_t)DP;
    float da = 0.f;
    for (int c = 0; c < dh; c += 8) {
      float vv[8];
      Vec<T, 8>::ld(vr + c, vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) da = fmaf(go[c + j], vv[j], da);
    }
    float x = da;
    if (kind != SGL_ATTN_GRAD_DP) {
      x = probs[bh * (size_t)N + n] * da;
      if (kind == SGL_ATTN_GRAD_RELEVANCE) x = x > 0.f ? x : (x != x ? x : 0.f);
    }
    acc += x;
  }
  if constexpr (MEAN) acc /= heads;
  out[idx] = acc;
}

hipError_t pool_attn_grad_probs(const void* V, int dtype, const float* probs, const float* dout, float* out, int B, int H,
                                int N, int dh, int DP, int kind, int mode, hipStream_t s) {
  if (B < 1 || H < 1 || N < 1 || dh < 8 || DP % 8 || dh % 8 || dh > DP) return hipErrorInvalidValue;
  if (mode != SGL_ATTN_PROBS_FULL && mode != SGL_ATTN_PROBS_HEAD_MEAN) return hipErrorInvalidValue;
  if (kind != SGL_ATTN_GRAD_DP && kind != SGL_ATTN_GRAD_PDP && kind != SGL_ATTN_GRAD_RELEVANCE) return hipErrorInvalidValue;
  const size_t total = (size_t)B * (mode ? 1 : H) * N;
  if ((total + 255) / 256 >= (1ull << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + 255) / 256));
  return pool_dispatch(dtype, [&](auto elem) {
    using T = decltype(elem);
    if (mode)
      hipLaunchKernelGGL((pool_attn_grad_probs_kernel<T, true>), grid, dim3(256), 0, s, (const T*)V, probs, dout, out, H, N,
                         dh, DP, total, (float)H, kind);
    else
      hipLaunchKernelGGL((pool_attn_grad_probs_kernel<T, false>), grid, dim3(256), 0, s, (const T*)V, probs, dout, out, H,
                         N, dh, DP, total, (float)H, kind);
  });
}

}  // namespace sgl
