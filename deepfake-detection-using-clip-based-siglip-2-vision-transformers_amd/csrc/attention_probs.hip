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
#include "attention.hip.h"

namespace sgl {

namespace {

// workgroup -> (z, query tile, key tile), key tile fastest: the workgroups of one query tile share its Q rows in L2
__device__ __forceinline__ void ap_tile(int nqt, int nkt, int& z, int& qt, int& kt) {
  unsigned pid = blockIdx.x;
  kt = (int)(pid % (unsigned)nkt);
  pid /= (unsigned)nkt;
  qt = (int)(pid % (unsigned)nqt);
  z = (int)(pid / (unsigned)nqt);
}
// Output slab z is one image whose heads hd = 0 .. H-1 are summed (MEAN) or one (image, head) pair (FULL), which head_rows
// addresses as head z of image 0.
template <bool MEAN>
__device__ __forceinline__ void ap_head(int z, int hd, int& b, int& h) {
  b = MEAN ? z : 0;
  h = MEAN ? hd : z;
}

// store C-tile registers: row0 + ctile_row(i, hh), column `col` (stored only where both are < N)
__device__ __forceinline__ void ap_store(float* __restrict__ out, size_t zbase, const f32x16& p, int row0, int hh, int col,
                                         int N) {
  if (col >= N) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = row0 + ctile_row(i, hh);
    if (row < N) out[zbase + (size_t)row * (size_t)N + (size_t)col] = p[i];
  }
}

// ---- score producers of the MFMA kernel: how a wave forms the 32 x 32 tile S = Q[q0 ..] · K[kb ..]ᵀ of one head
// (A = Q, B = K, row = lane & 31 = li, lane half hh) and a probability from a score and the row's lse term.
// 16-bit operands: 16-byte fragments through the buffer bounds check (rows >= N read as zeros), v_mfma_f32_32x32x16, and
// exp2(S * c + L) with L = -lse * log2e, the fused multiply-add of the backward kernels of attention.hip.
template <typename T, int DPC>
struct ProbsLo {
  using elem = T;
  static constexpr int KS = DPC / 16, dp_const = DPC;
  __amdgpu_buffer_rsrc_t rq, rk;
  lo_x8<T> qf[KS];
  static __device__ __forceinline__ lo_x8<T> frag(__amdgpu_buffer_rsrc_t r, int row, int N, int ks, int hh) {
    return __builtin_bit_cast(
        lo_x8<T>, __builtin_amdgcn_raw_buffer_load_b128(
                      r, (row < N) ? (uint32_t)row * (uint32_t)(DPC * 2) + (uint32_t)(2 * ks + hh) * 16u : SGL_OOB, 0, 0));
  }
  __device__ __forceinline__ void head(const T* Qh, const T* Kh, int N, int dh, int rs, int qrow, int hh) {
    const uint32_t hbytes = (uint32_t)((size_t)N * DPC * 2);
    rq = make_rsrc(Qh, hbytes);
    rk = make_rsrc(Kh, hbytes);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = frag(rq, qrow, N, ks, hh);
  }
  __device__ __forceinline__ f32x16 scores(int krow, int N, int hh) const {
    lo_x8<T> kf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kf[ks] = frag(rk, krow, N, ks, hh);
    f32x16 S;
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) S = mfma_32x32x16(qf[ks], kf[ks], S);
    return S;
  }
  static __device__ __forceinline__ float lse_term(float lse) { return -lse * kLog2e; }
  static __device__ __forceinline__ float prob(float S, float c, float L) { return __builtin_amdgcn_exp2f(fmaf(S, c, L)); }
};
// fp32 operands on v_mfma_f32_32x32x2_f32: A[m][k] from lane (m = lane & 31, k = lane >> 5), B[k][n] likewise; scalar loads,
// k-steps in ascending order and expf(S * scale - lse) as attention_f32.hip.
struct ProbsF32 {
  using elem = float;
  static constexpr int dp_const = 0;   // head_dim_pad is a runtime value
  const float *qrow, *Kh;
  int ks, rs, hh;
  bool qok;
  __device__ __forceinline__ void head(const float* Qh, const float* Kh_, int N, int dh, int rs_, int qr, int hh_) {
    ks = dh / 2, rs = rs_, hh = hh_, Kh = Kh_;
    qok = qr < N;
    qrow = Qh + (size_t)(qok ? qr : 0) * rs + hh;
  }
  __device__ __forceinline__ f32x16 scores(int kr, int N, int) const {
    const bool kok = kr < N;
    const float* krow = Kh + (size_t)(kok ? kr : 0) * rs + hh;
    f32x16 S;
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] = 0.f;
    for (int s = 0; s < ks; ++s) {
      const float a = qok ? qrow[2 * s] : 0.f;
      const float b = kok ? krow[2 * s] : 0.f;
      S = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, S, 0, 0, 0);
    }
    return S;
  }
  static __device__ __forceinline__ float lse_term(float lse) { return lse; }
  static __device__ __forceinline__ float prob(float S, float scale, float L) { return expf(S * scale - L); }
};

// A workgroup of 4 waves owns a 128 x 128 tile of slab z; wave w owns query rows 32w .. 32w+31 and the four 32-key sub-tiles.
// c: the factor P::prob multiplies a score by (log2e / sqrt(dh) for ProbsLo, 1 / sqrt(dh) for ProbsF32).
template <typename P, bool MEAN>
__global__ __launch_bounds__(256) void attn_probs_kernel(const typename P::elem* __restrict__ Q,
                                                         const typename P::elem* __restrict__ K,
                                                         const float* __restrict__ lse, float* __restrict__ out, int H,
                                                         int N, int dh, int DP, int nqt, int nkt, float c, float heads) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, hh = lane >> 5;
  int z, qt, kt;
  ap_tile(nqt, nkt, z, qt, kt);
  const int q0 = qt * 128 + w * 32, k0 = kt * 128;
  if (q0 >= N) return;   // wave-uniform; the kernel has no barrier
  const int nh = MEAN ? H : 1;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  const size_t zbase = (size_t)z * (size_t)N * (size_t)N;

  for (int hd = 0; hd < nh; ++hd) {
    int b, h, rs;
    ap_head<MEAN>(z, hd, b, h);
    const size_t bh = (size_t)b * H + h;
    const size_t base = head_rows(0, b, h, H, N, dh, P::dp_const ? P::dp_const : DP, rs);
    P p;
    p.head(Q + base, K + base, N, dh, rs, q0 + li, hh);
    float L[16];   // the lse term of this lane's 16 query rows
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = q0 + ctile_row(i, hh);
      L[i] = (row < N) ? P::lse_term(lse[bh * (size_t)N + row]) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kb = k0 + 32 * j;
      if (kb < N) {   // wave-uniform
        f32x16 S = p.scores(kb + li, N, hh);
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i] = P::prob(S[i], c, L[i]);
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
    int b, h, rs;
    ap_head<MEAN>(z, hd, b, h);
    const size_t bh = (size_t)b * H + h;
    const size_t base = head_rows(0, b, h, H, N, dh, DP, rs);
    const float* qr = Q + base + (size_t)row * rs;
    const float* kr = K + base + (size_t)col * rs;
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

}  // namespace

bool attn_probs_shape_ok(int dtype, int B, int H, int N, int dh, int DP) {
  return attn_shape_ok(dtype, B, H, N, dh, DP, 0, ATTN_PROBS);
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
  if (!attn_shape_ok(dtype, B, H, N, dh, DP, 0, ATTN_PROBS)) return hipErrorInvalidValue;
  if (mode != SGL_ATTN_PROBS_FULL && mode != SGL_ATTN_PROBS_HEAD_MEAN) return hipErrorInvalidValue;
  const size_t Z = mode ? B : B * H;
  const AttnScales sc = attn_scales(dh);
  const float heads = (float)H;
  // nqt x nkt tiles per output slab; `elem` carries the kernel's operand type
  auto launch = [&](auto kernel, auto elem, int nqt, int nkt, float c) {
    using E = decltype(elem);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((size_t)nqt * nkt * Z)), dim3(256), 0, s, (const E*)q, (const E*)k, lse,
                       out, H, N, dh, DP, nqt, nkt, c, heads);
    return hipGetLastError();
  };
  const int nt = (N + 127) / 128;
  return with_bool(mode != 0, [&](auto mean) -> hipError_t {
    constexpr bool MEAN = mean.value;
    if (dtype == DT_F32)
      return launch(attn_probs_ref_kernel<MEAN>, 0.f, (N + 3) / 4, (N + 63) / 64, sc.scale);
    if (dtype == DT_F32_MFMA)
      return launch(attn_probs_kernel<ProbsF32, MEAN>, 0.f, nt, nt, sc.scale);
    if ((dtype != DT_BF16 && dtype != DT_F16) || !attn_aligned16(q, k)) return hipErrorInvalidValue;
    return dispatch_attn(dtype, DP, [&](auto tag) {
      using T = typename decltype(tag)::type;
      return launch(attn_probs_kernel<ProbsLo<T, decltype(tag)::dp>, MEAN>, T{}, nt, nt, sc.c);
    });
  });
}

}  // namespace sgl
