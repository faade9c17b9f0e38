// Fused GEMM epilogues, applied to NV consecutive output columns of one row (row-contiguous so that bias,
// residual and output traffic is 16-byte vectorised).  Shared by the MFMA kernels (NV = 8, after the
// accumulator tile has been transposed through LDS) and the strict-fp32 generic kernel (NV = 4).
//
// Reference ops being fused (TF:models/siglip/modeling_siglip.py):
//   EPI_QKV       q/k/v_proj bias + view(B,N,H,dh).transpose(1,2)            :284-286
//   EPI_RES_F32   out_proj / fc2 bias + residual add                        :303-304,349,354
//   EPI_BIAS_GELU fc1 bias + gelu_pytorch_tanh                              :319-320
//   EPI_POS_F32   patch conv bias + position embedding add                  :178-184
#pragma once
#include <type_traits>

#include "common.hip.h"
#include "kernels.h"

namespace sgl {

// The value arithmetic and the stores of the four epilogues that have operands besides an optional bias, on NV
// consecutive columns of one row.  The caller supplies the operands and the destinations: epi_apply below loads and
// addresses per chunk; the staged epilogue of gemm_bf16_v2.hip loads the bias once per thread, requests the residual /
// pre-activation one pass ahead and keeps the column part of the QKV address per thread.
template <int NV>
__device__ __forceinline__ void epi_res_f32(float* v, const float* bias, const float* r, float* dst) {
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = r[j] + (v[j] + bias[j]);
  Vec<float, NV>::st_nt(dst, v);
}
// dst_u (inside p.out) is written only when p.out is given: the pre-activation u (or gelu'(u),
// EpiParams::gelu_grad_form) is only read by the backward GELU'; inference and frozen blocks pass out == nullptr
template <typename TOut, int NV>
__device__ __forceinline__ void epi_bias_gelu(const EpiParams& p, float* v, const float* bias, TOut* dst_u, TOut* dst_act) {
  float a[NV];
  if (p.out && p.gelu_grad_form) {   // training, derivative form: out := gelu'(u)
#pragma unroll
    for (int j = 0; j < NV; ++j) gelu_tanh_both(v[j] + bias[j], a[j], v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      v[j] += bias[j];
      a[j] = gelu_tanh(v[j]);
    }
  }
  if (p.out) Vec<TOut, NV>::st_nt(dst_u, v);
  Vec<TOut, NV>::st_nt(dst_act, a);
}
// row -> (b, n) = (row / tokens, row % tokens) without the ~35-instruction integer division (16 of them per thread and
// tile otherwise): float reciprocal estimate, then one exact correction step (rows < 2^22)
__device__ __forceinline__ void qkv_split_row(int row, int tokens, int& b, int& n) {
  b = (int)((float)row * __builtin_amdgcn_rcpf((float)tokens));
  n = row - b * tokens;
  if (n < 0) { b -= 1; n += tokens; }
  else if (n >= tokens) { b += 1; n -= tokens; }
}
// pad_chunks: NV-chunks of zeros behind the head's last data chunk, the pad columns [head_dim, head_dim_pad).
// head_dim % 8 == 0 and head_dim_pad = round_up(head_dim, 16), so the pad is 0 or 8 elements, i.e. whole NV-chunks:
// vector stores (scalar 2-byte stores here cost the QKV GEMM ~15 %)
template <typename TOut, int NV>
__device__ __forceinline__ void epi_qkv(float* v, const float* bias, TOut* dst, int pad_chunks) {
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] += bias[j];
  Vec<TOut, NV>::st_nt(dst, v);
  if (pad_chunks) {
    float z[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) z[j] = 0.f;
    for (int k = 1; k <= pad_chunks; ++k) Vec<TOut, NV>::st_nt(dst + k * NV, z);
  }
}
// One 16-byte chunk of the head-major QKV walk (store_tile_qkv_heads, gemm_bf16_v2.hip): the chunk's eight values, bias
// already added, arrive as two halves read from LDS in either order (`swapped`: `first` holds columns 4..7; the order is
// what keeps those reads free of bank conflicts), are rounded like Vec<TOut, 8>::st_nt rounds them and leave as one
// streaming store.  `pad`: a chunk of the columns [head_dim, head_dim_pad), stored as +0 in-stream with the data chunks
// round it instead of by a second, branched store.
template <typename TOut>
__device__ __forceinline__ void epi_qkv_halves(f32x4 first, f32x4 second, bool swapped, bool pad, TOut* dst) {
  static_assert(sizeof(TOut) == 2, "16-bit outputs: eight columns are one 16-byte chunk");
  lo_x4<TOut> pf, ps;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    pf[j] = (TOut)first[j];
    ps[j] = (TOut)second[j];
  }
  const u32x2 uf = __builtin_bit_cast(u32x2, pf), us = __builtin_bit_cast(u32x2, ps);
  const u32x2 lo = swapped ? us : uf, hi = swapped ? uf : us;
  u32x4 o = {lo[0], lo[1], hi[0], hi[1]};
  if (pad) o = u32x4{0u, 0u, 0u, 0u};
  __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(dst));
}
// u: the saved pre-activation, or gelu'(u) itself with EpiParams::gelu_grad_form; leaves the stored values in v
template <typename TOut, int NV>
__device__ __forceinline__ void epi_gelu_bwd(const EpiParams& p, float* v, const float* u, TOut* dst) {
  if (p.gelu_grad_form) {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] *= u[j];
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] *= gelu_tanh_grad(u[j]);
  }
  Vec<TOut, NV>::st_nt(dst, v);
}

// Workgroup barrier that orders LDS traffic only: raw s_barrier + lgkmcnt(0).  __syncthreads() would also emit vmcnt(0)
// and make the caller wait for its global stores to be acknowledged (microseconds under load); they stay in flight.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Fused bias gradient of EPI_GELU_BWD, after the chunk loop of a workgroup of NT threads on a tile BN columns wide: every
// thread owns the same NV columns in all its chunks (NT % (BN / NV) == 0) and has their sums over its rows in csum.  Folds
// the NT / (BN / NV) row groups through LDS (ct: at least NT * NV floats, free to overwrite) and gives one value per
// column to p.colsum (EpiParams: stored per 128-row block when colsum_ld > 0, added atomically otherwise).
template <int NT, int BN, int NV>
__device__ __forceinline__ void epi_colsum_fold(float* ct, const float (&csum)[NV], int t, int m0, int n0, int N,
                                                const EpiParams& p) {
  constexpr int CPR = BN / NV, GROUPS = NT / CPR;
  static_assert(NT % CPR == 0 && BN <= NT, "one fixed column set per thread, one thread per column");
  if (!p.colsum) return;
  lds_barrier();
#pragma unroll
  for (int j = 0; j < NV; ++j) ct[(t / CPR) * BN + (t % CPR) * NV + j] = csum[j];
  lds_barrier();
  if (t < BN && n0 + t < N) {
    float s = 0.f;
#pragma unroll
    for (int gI = 0; gI < GROUPS; ++gI) s += ct[gI * BN + t];
    if (p.colsum_ld > 0)
      p.colsum[(size_t)(m0 >> 7) * p.colsum_ld + n0 + t] = s;
    else
      atomicAdd(p.colsum + n0 + t, s);
  }
}

template <int EPI, typename TOut, int NV>
__device__ __forceinline__ void epi_apply(const EpiParams& p, int row, int col, int N, float* v) {
  if constexpr (EPI == EPI_STORE) {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] *= p.alpha;
    if (p.bias) {
      float b[NV];
      Vec<float, NV>::ld(p.bias + col, b);
#pragma unroll
      for (int j = 0; j < NV; ++j) v[j] += b[j];
    }
    Vec<TOut, NV>::st_nt(reinterpret_cast<TOut*>(p.out) + (size_t)row * p.ldo + col, v);
  } else if constexpr (EPI == EPI_BIAS_GELU) {
    float b[NV];
    Vec<float, NV>::ld(p.bias + col, b);
    epi_bias_gelu<TOut, NV>(p, v, b, reinterpret_cast<TOut*>(p.out) + (size_t)row * p.ldo + col,
                            reinterpret_cast<TOut*>(p.out2) + (size_t)row * p.ldo2 + col);
  } else if constexpr (EPI == EPI_RES_F32) {
    float b[NV], r[NV];
    Vec<float, NV>::ld(p.bias + col, b);
    Vec<float, NV>::ld(p.res + (size_t)row * p.ldr + col, r);
    epi_res_f32<NV>(v, b, r, reinterpret_cast<float*>(p.out) + (size_t)row * p.ldo + col);
  } else if constexpr (EPI == EPI_QKV) {
    const int dm = p.heads * p.head_dim;
    const int which = col / dm;
    const int hc = col - which * dm;
    const int h = hc / p.head_dim;
    const int d = hc - h * p.head_dim;
    int b, n;
    qkv_split_row(row, p.tokens, b, n);
    float bb[NV];
    Vec<float, NV>::ld(p.bias + col, bb);
    TOut* dst = reinterpret_cast<TOut*>(p.out) +
                ((((size_t)which * p.batch + b) * p.heads + h) * p.tokens + n) * p.head_dim_pad + d;
    epi_qkv<TOut, NV>(v, bb, dst, (d + NV == p.head_dim) ? (p.head_dim_pad - p.head_dim) / NV : 0);
  } else if constexpr (EPI == EPI_GELU_BWD) {
    float u[NV];
    Vec<TOut, NV>::ld(reinterpret_cast<const TOut*>(p.aux) + (size_t)row * p.ldaux + col, u);
    epi_gelu_bwd<TOut, NV>(p, v, u, reinterpret_cast<TOut*>(p.out) + (size_t)row * p.ldo + col);
  } else if constexpr (EPI == EPI_POS_F32) {
    float b[NV], e[NV];
    Vec<float, NV>::ld(p.bias + col, b);
    Vec<float, NV>::ld(p.pos + (size_t)(row % p.pos_rows) * N + col, e);
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = (v[j] + b[j]) + e[j];
    Vec<float, NV>::st(reinterpret_cast<float*>(p.out) + (size_t)row * p.ldo + col, v);
  } else {  // EPI_F32
    float* dst = reinterpret_cast<float*>(p.out) + (size_t)row * p.ldo + col;
    const int nv = (col + NV <= N) ? NV : (N - col);
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] *= p.alpha;
    if (p.bias) {
      for (int j = 0; j < nv; ++j) v[j] += p.bias[col + j];
    }
    if (p.atomic) {
      for (int j = 0; j < nv; ++j) atomicAdd(dst + j, v[j]);
    } else if (nv == NV && (p.ldo % NV) == 0) {
      if (p.accumulate) {
        float o[NV];
        Vec<float, NV>::ld(dst, o);
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] += o[j];
      }
      Vec<float, NV>::st(dst, v);
    } else {
      for (int j = 0; j < nv; ++j) dst[j] = p.accumulate ? dst[j] + v[j] : v[j];
    }
  }
}

// Host side: calls launch(EpiTag<EPI, TOut>{}) for a runtime (epilogue, output dtype) pair, so that every GEMM family
// instantiates the same table: bf16 (fp16) or fp32 outputs for the first four epilogues (fp32 = bf16x3 strict mode on the MFMA
// kernels), fp32 for the others.
template <int EPI, typename TOut>
struct EpiTag {
  static constexpr int epi = EPI;
  using out = TOut;
};
// TLo is the 16-bit output type of the family being dispatched (bf16, or fp16 for the DT_F16 kernels): out_dtype selects
// it or fp32.
template <typename TLo = bf16, typename Launch>
hipError_t dispatch_epilogue(int epi, int out_dtype, Launch&& launch) {
  const bool b16 = out_dtype == (std::is_same<TLo, f16>::value ? DT_F16 : DT_BF16);
  switch (epi) {
    case EPI_STORE: return b16 ? launch(EpiTag<EPI_STORE, TLo>{}) : launch(EpiTag<EPI_STORE, float>{});
    case EPI_BIAS_GELU: return b16 ? launch(EpiTag<EPI_BIAS_GELU, TLo>{}) : launch(EpiTag<EPI_BIAS_GELU, float>{});
    case EPI_QKV: return b16 ? launch(EpiTag<EPI_QKV, TLo>{}) : launch(EpiTag<EPI_QKV, float>{});
    case EPI_GELU_BWD: return b16 ? launch(EpiTag<EPI_GELU_BWD, TLo>{}) : launch(EpiTag<EPI_GELU_BWD, float>{});
    case EPI_RES_F32: return launch(EpiTag<EPI_RES_F32, float>{});
    case EPI_POS_F32: return launch(EpiTag<EPI_POS_F32, float>{});
    case EPI_F32: return launch(EpiTag<EPI_F32, float>{});
  }
  return hipErrorInvalidValue;
}

}  // namespace sgl
