// What the attention translation units (attention.hip, attention_f32.hip, attention_ref.hip, attention_probs.hip) must
// agree on, written once: where a head lives in a q/k/v source, which shapes each route takes, how a runtime
// (dtype, head_dim_pad) pair becomes a kernel instantiation, the softmax constants, and the internal launchers' signatures.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.hip.h"
#include "kernels.h"

namespace sgl {

// ---- constants ------------------------------------------------------------------------------------------------------
constexpr float kLog2e = SGL_LOG2E;
// scale = 1/sqrt(dh); c = scale * log2e, the factor of the exp2-based softmax of the 16-bit kernels
struct AttnScales {
  float scale, c;
};
static inline AttnScales attn_scales(int dh) {
  const float scale = 1.0f / sqrtf((float)dh);
  return {scale, scale * kLog2e};
}

// Row of the 32x32 MFMA C tile that accumulator register i holds in lane half hh = lane >> 5 (the column is lane & 31).
__host__ __device__ constexpr int ctile_row(int i, int hh) { return 8 * (i >> 2) + 4 * hh + (i & 3); }

// ---- head addressing ------------------------------------------------------------------------------------------------
// Where head (b, hd) lives in a q/k/v source: token-major [B*N][ld] column blocks (ld > 0) or head-major [B][H][N][DP]
// (ld == 0).  `base` is the element offset of (token 0, column 0) of the head.  The other three fields serve the 16-bit
// kernels' buffer descriptors: byte stride between token rows, 16-byte data chunks per row, buffer extent in bytes.
// These statements are the addressing of the three hot 16-bit kernels, whose code is pinned instruction for instruction:
// reordering them, or moving one into a helper, reorders the kernels' scalar prologues.
struct HeadSrc {
  uint32_t rowbytes, nc, bytes;
  size_t base;
};
__device__ __forceinline__ HeadSrc head_src(int ld, int b, int hd, int H, int N, int dh, int DP) {
  HeadSrc r;
  if (ld > 0) {
    r.rowbytes = (uint32_t)ld * 2u;
    r.nc = (uint32_t)dh / 8u;
    r.bytes = (uint32_t)(((size_t)(N - 1) * ld + dh) * 2);
    r.base = (size_t)b * N * ld + (size_t)hd * dh;
  } else {
    r.rowbytes = (uint32_t)DP * 2u;
    r.nc = (uint32_t)DP / 8u;
    r.bytes = (uint32_t)((size_t)N * DP * 2);
    r.base = ((size_t)b * H + hd) * (size_t)N * DP;
  }
  return r;
}
// The dtype-independent view of the same: the head's element offset and the element stride between its token rows.
__device__ __forceinline__ size_t head_rows(int ld, int b, int h, int H, int N, int dh, int DP, int& row_stride) {
  row_stride = ld > 0 ? ld : DP;
  return head_src(ld, b, h, H, N, dh, DP).base;
}

// ---- ragged (varlen) addressing ---------------------------------------------------------------------------------------
// Packed layout of the *_varlen kernels: segment s owns rows cu[s] .. cu[s+1]-1 of every [T]-row buffer, q/k/v are
// head-major [H][T][DP].  A workgroup serves one (segment, head) pair and one block of `rows` query rows of it; the 1-D
// launch and the XCD map are head_block's of attention.hip (XCD x owns pairs x, x+8, ...; 8 * ceil(S*H / 8) * nb
// workgroups).  What is read from cu is clamped: 0 <= row0 <= row0 + n <= T and n <= max_n, so a wrong table gives wrong
// numbers and never an address outside the buffers.  False: a padding pair, or a block that starts past the segment's end
// (the whole workgroup returns before its first barrier).
struct SegBlock {
  int seg, hd, xb;   // segment, head, block index within the segment
  int row0, n;       // first row of the segment in the packed buffers, its token count
};
// the clamp: rows [row0, row0 + n) of segment seg < S
__device__ __forceinline__ void seg_range(const int* __restrict__ cu, int seg, int T, int max_n, int& row0, int& n) {
  const int lo = min(max(cu[seg], 0), T);
  const int hi = min(max(cu[seg + 1], lo), T);
  row0 = lo;
  n = min(hi - lo, max_n);
}
__device__ __forceinline__ bool seg_block(const int* __restrict__ cu, int S, int T, int max_n, int H, int nb, int rows,
                                          SegBlock& sb) {
  const int pid = blockIdx.x, xcd = pid & 7, slot = pid >> 3;
  const int hq = slot / nb;
  const int sh = hq * 8 + xcd;
  if (sh >= S * H) return false;
  sb.xb = slot - hq * nb;
  sb.seg = sh / H;
  sb.hd = sh - sb.seg * H;
  seg_range(cu, sb.seg, T, max_n, sb.row0, sb.n);
  return sb.xb * rows < sb.n;
}
static inline dim3 seg_grid(int nb, int SH) { return dim3((unsigned)(8 * ((SH + 7) / 8) * nb)); }
// S * H pairs times nb blocks in a 1-D grid
static inline bool seg_grid_ok(int S, int H, int nb) { return (size_t)8 * (((size_t)S * H + 7) / 8) * (size_t)nb < (1ull << 31); }

// ---- the shape contract ---------------------------------------------------------------------------------------------
// head_dim_pad values of the 16-bit kernels: the contract accepts exactly these and dispatch_attn instantiates exactly these
constexpr int kAttnDP[] = {16, 32, 48, 64, 80, 96};
constexpr int kAttnNDP = sizeof(kAttnDP) / sizeof(kAttnDP[0]);
constexpr bool attn_dp_ok(int DP) {
  for (int i = 0; i < kAttnNDP; ++i)
    if (kAttnDP[i] == DP) return true;
  return false;
}
// strict route (DT_F32): dynamic LDS of a workgroup, 4 waves x (nvec score vectors of N floats + nrow staged 128-float rows)
constexpr size_t attn_ref_lds(int N, int nvec, int nrow) { return (size_t)4 * (nvec * N + 128 * nrow) * sizeof(float); }

enum AttnPass : int { ATTN_FWD, ATTN_BWD, ATTN_PROBS };
// Every shape rule of attention, per dtype route (DT_F32 strict, DT_F32_MFMA, anything else 16-bit); ld = 0 for ATTN_PROBS.
// attn_fwd, attn_bwd and attn_probs refuse with hipErrorInvalidValue what this refuses.  Defined in attention.hip.
bool attn_shape_ok(int dtype, int B, int H, int N, int dh, int DP, int ld, AttnPass pass);
// the 16-bit kernels fetch 16 bytes per lane from these
static inline bool attn_aligned16(const void* a, const void* b, const void* c = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0;
}

// ---- dispatch -------------------------------------------------------------------------------------------------------
// Calls f(AttnTag<T, DP>{}) for the 16-bit operand type of `dtype` (DT_F16: f16, anything else bf16) and a head_dim_pad of
// kAttnDP; hipErrorInvalidValue for any other DP.  The 16-bit sibling of dispatch_epilogue (epilogue.hip.h).
template <typename T, int DP>
struct AttnTag {
  using type = T;
  static constexpr int dp = DP;
};
template <typename T, int I = 0, typename F>
hipError_t dispatch_attn_dp(int DP, F&& f) {
  if constexpr (I == kAttnNDP) {
    return hipErrorInvalidValue;
  } else {
    if (DP == kAttnDP[I]) return f(AttnTag<T, kAttnDP[I]>{});
    return dispatch_attn_dp<T, I + 1>(DP, f);
  }
}
template <typename F>
hipError_t dispatch_attn(int dtype, int DP, F&& f) {
  return dtype == DT_F16 ? dispatch_attn_dp<f16>(DP, f) : dispatch_attn_dp<bf16>(DP, f);
}
// f(std::true_type / std::false_type): a runtime flag as a template boolean (the kernels' TOK and MEAN)
template <typename F>
auto with_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// ---- internal launchers (attention_f32.hip, attention_ref.hip); the caller has checked attn_shape_ok -------------------
// delta: scratch of B*H*N floats (the caller's 2*B*H*N buffer is more than enough)
hipError_t attn_f32_fwd(const float* q, const float* k, const float* v, float* out, float* lse, int B, int H, int N, int dh,
                        int DP, int ld, hipStream_t s);
hipError_t attn_f32_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout,
                        const float* lse, float* dqkv, float* delta, int B, int H, int N, int dh, int DP, int ld,
                        hipStream_t s);
hipError_t attn_ref_fwd(const float* q, const float* k, const float* v, float* out, float* lse, int B, int H, int N, int dh,
                        int DP, int ld, hipStream_t s);
hipError_t attn_ref_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout,
                        const float* lse, float* dqkv, float* delta, int B, int H, int N, int dh, int DP, int ld,
                        hipStream_t s);
// the ragged forwards of the two fp32 routes (attn_fwd_varlen has checked the shapes): q, k, v [H][T][DP], cu on the device
hipError_t attn_f32_fwd_varlen(const float* q, const float* k, const float* v, float* out, float* lse, const int* cu, int S,
                               int T, int max_n, int H, int dh, int DP, hipStream_t s);
hipError_t attn_ref_fwd_varlen(const float* q, const float* k, const float* v, float* out, float* lse, const int* cu, int S,
                               int T, int max_n, int H, int dh, int DP, hipStream_t s);

}  // namespace sgl
