// Gradient of a score with respect to the attention probabilities of one block, and its products with them, formed at the
// one point of the backward where every operand exists: the head-major q, k, v and the row log-sum-exp a saving forward
// keeps, and dO, the gradient of the attention output (token-major [B*N][H*dh], what attn_bwd takes).
//   dP[b,h,i,j] = sum_d dO[b,i,h*dh+d] * V[b,h,j,d]          (the .grad autograd gives an eager softmax(QK^T) V)
//   P[b,h,i,j]  = the expression of attention_probs.hip: same operands, constants and exp2(fma) / expf per route
//   kind DP         x = dP
//        PDP        x = P * dP
//        RELEVANCE  x = relu(P * dP) with a NaN kept: x > 0 ? x : (x != x ? x : 0).  fmaxf(x, 0) would return 0 for a
//                   NaN and hide an overflowing pass, which the non-finite contract forbids.
//   mode FULL       out (B,H,N,N) fp32;  HEAD_MEAN  out (B,N,N) fp32 = (sum_h x[b,h]) / H, heads summed in ascending order in
//                   registers, one IEEE division by H, one store (as attention_probs.hip): the per-head tensor never exists.
// Every input is const; no atomics, no LDS, no barriers; each output element is written by exactly one 4-byte store, so a
// call is bitwise reproducible.  Rows / keys >= N are never stored.
//
// 16-bit kernel: the tiling of attn_probs_kernel.  A workgroup of 4 waves owns a 128 x 128 tile of one output slab; wave w
// owns query rows 32w .. 32w+31 and the four 32-key sub-tiles.  Per head the wave holds the Q and the dO fragments of its 32
// rows; per sub-tile it fetches the K and V fragments and forms S = Q K^T and dP = dO V^T on v_mfma_f32_32x32x16_{bf16,f16}
// (A = Q / dO, B = K / V, 16 bytes per lane straight from global memory through the buffer bounds check).
// Head h of dO starts at column h * dh of a row of H * dh: with dh = 72, DP = 80 the upper 16-byte chunk of the last k-step
// lies in head h + 1.  It is read as zero through the bounds check (chunk index >= dh / 8), never multiplied by V's zero
// pad: NaN * 0 would carry a neighbour head's non-finite into this head.  dh % 8 == 0 makes chunk granularity sufficient.
// fp32 operands: v_mfma_f32_32x32x2_f32 over the dh real columns, k-steps ascending (SGL_DTYPE_BF16X3's route), or one
// thread per element with one FMA chain per product (F32); neither is a performance path.
#include "attention.hip.h"

namespace sgl {

namespace {

// workgroup -> (z, query tile, key tile), key tile fastest (attention_probs.hip)
__device__ __forceinline__ void ag_tile(int nqt, int nkt, int& z, int& qt, int& kt) {
  unsigned pid = blockIdx.x;
  kt = (int)(pid % (unsigned)nkt);
  pid /= (unsigned)nkt;
  qt = (int)(pid % (unsigned)nqt);
  z = (int)(pid / (unsigned)nqt);
}
// output slab z: one image whose heads hd = 0 .. H-1 are summed (MEAN) or one (image, head) pair (FULL)
template <bool MEAN>
__device__ __forceinline__ void ag_head(int z, int hd, int H, int& b, int& h) {
  b = MEAN ? z : z / H;
  h = MEAN ? hd : z % H;
}

__device__ __forceinline__ float ag_combine(int kind, float p, float dp) {
  if (kind == SGL_ATTN_GRAD_DP) return dp;
  const float x = p * dp;
  if (kind == SGL_ATTN_GRAD_PDP) return x;
  return x > 0.f ? x : (x != x ? x : 0.f);
}

__device__ __forceinline__ void ag_store(float* __restrict__ out, size_t zbase, const f32x16& p, int row0, int hh, int col,
                                         int N) {
  if (col >= N) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = row0 + ctile_row(i, hh);
    if (row < N) out[zbase + (size_t)row * (size_t)N + (size_t)col] = p[i];
  }
}

// ---- tile producers: how a wave forms S = Q[q0 ..] K[kb ..]^T and dP = dO[q0 ..] V[kb ..]^T of one head ------------------
template <typename T, int DPC>
struct GradLo {
  using elem = T;
  static constexpr int KS = DPC / 16, dp_const = DPC;
  __amdgpu_buffer_rsrc_t rq, rk, rv;
  lo_x8<T> qf[KS], gf[KS];
  // head-major row of DPC elements
  static __device__ __forceinline__ lo_x8<T> frag(__amdgpu_buffer_rsrc_t r, int row, int N, int ks, int hh) {
    return __builtin_bit_cast(
        lo_x8<T>, __builtin_amdgcn_raw_buffer_load_b128(
                      r, (row < N) ? (uint32_t)row * (uint32_t)(DPC * 2) + (uint32_t)(2 * ks + hh) * 16u : SGL_OOB, 0, 0));
  }
  __device__ __forceinline__ void head(const T* Qh, const T* Kh, const T* Vh, const T* dO, int b, int h, int H, int N,
                                       int dh, int rs, int qrow, int hh, bool want_p) {
    const uint32_t hbytes = (uint32_t)((size_t)N * DPC * 2);
    rq = make_rsrc(Qh, hbytes);
    rk = make_rsrc(Kh, hbytes);
    rv = make_rsrc(Vh, hbytes);
    // dO of head (b, h): rows of H * dh elements, dh / 8 chunks of which are this head's
    const HeadSrc g = head_src(H * dh, b, h, H, N, dh, DPC);
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(dO + g.base, g.bytes);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint32_t ch = (uint32_t)(2 * ks + hh);
      gf[ks] = __builtin_bit_cast(
          lo_x8<T>, __builtin_amdgcn_raw_buffer_load_b128(
                        rg, (qrow < N && ch < g.nc) ? (uint32_t)qrow * g.rowbytes + ch * 16u : SGL_OOB, 0, 0));
    }
    if (want_p) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) qf[ks] = frag(rq, qrow, N, ks, hh);
    }
  }
  __device__ __forceinline__ f32x16 scores(int krow, int N, int hh) const {
    f32x16 S;
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) S = mfma_32x32x16(qf[ks], frag(rk, krow, N, ks, hh), S);
    return S;
  }
  __device__ __forceinline__ f32x16 dprobs(int krow, int N, int hh) const {
    f32x16 S;
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) S = mfma_32x32x16(gf[ks], frag(rv, krow, N, ks, hh), S);
    return S;
  }
  static __device__ __forceinline__ float lse_term(float lse) { return -lse * kLog2e; }
  static __device__ __forceinline__ float prob(float S, float c, float L) { return __builtin_amdgcn_exp2f(fmaf(S, c, L)); }
};
// fp32 operands on v_mfma_f32_32x32x2_f32: A[m][k] from lane (m = lane & 31, k = lane >> 5), B[k][n] likewise; scalar loads
// over the dh real columns only, so no pad column of any operand is touched
struct GradF32 {
  using elem = float;
  static constexpr int dp_const = 0;   // head_dim_pad is a runtime value
  const float *qrow, *grow, *Kh, *Vh;
  int ks, rs, hh;
  bool qok;
  __device__ __forceinline__ void head(const float* Qh, const float* Kh_, const float* Vh_, const float* dO, int b, int h,
                                       int H, int N, int dh, int rs_, int qr, int hh_, bool) {
    ks = dh / 2, rs = rs_, hh = hh_, Kh = Kh_, Vh = Vh_;
    qok = qr < N;
    qrow = Qh + (size_t)(qok ? qr : 0) * rs + hh;
    grow = dO + ((size_t)b * N + (qok ? qr : 0)) * ((size_t)H * dh) + (size_t)h * dh + hh;
  }
  __device__ __forceinline__ f32x16 product(const float* arow, const float* Bh, int kr, int N) const {
    const bool kok = kr < N;
    const float* brow = Bh + (size_t)(kok ? kr : 0) * rs + hh;
    f32x16 S;
#pragma unroll
    for (int i = 0; i < 16; ++i) S[i] = 0.f;
    for (int s = 0; s < ks; ++s) {
      const float a = qok ? arow[2 * s] : 0.f;
      const float b = kok ? brow[2 * s] : 0.f;
      S = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, S, 0, 0, 0);
    }
    return S;
  }
  __device__ __forceinline__ f32x16 scores(int kr, int N, int) const { return product(qrow, Kh, kr, N); }
  __device__ __forceinline__ f32x16 dprobs(int kr, int N, int) const { return product(grow, Vh, kr, N); }
  static __device__ __forceinline__ float lse_term(float lse) { return lse; }
  static __device__ __forceinline__ float prob(float S, float scale, float L) { return expf(S * scale - L); }
};

// c: the factor G::prob multiplies a score by (log2e / sqrt(dh) for GradLo, 1 / sqrt(dh) for GradF32).  `kind` is uniform
// over the launch: DP skips the Q fragments, the score MFMAs and the exponentials.
template <typename G, bool MEAN>
__global__ __launch_bounds__(256) void attn_grad_probs_kernel(const typename G::elem* __restrict__ Q,
                                                              const typename G::elem* __restrict__ K,
                                                              const typename G::elem* __restrict__ V,
                                                              const typename G::elem* __restrict__ dO,
                                                              const float* __restrict__ lse, float* __restrict__ out,
                                                              int H, int N, int dh, int DP, int nqt, int nkt, float c,
                                                              float heads, int kind) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, hh = lane >> 5;
  int z, qt, kt;
  ag_tile(nqt, nkt, z, qt, kt);
  const int q0 = qt * 128 + w * 32, k0 = kt * 128;
  if (q0 >= N) return;   // wave-uniform; the kernel has no barrier
  const int nh = MEAN ? H : 1;
  const bool want_p = kind != SGL_ATTN_GRAD_DP;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  const size_t zbase = (size_t)z * (size_t)N * (size_t)N;

  for (int hd = 0; hd < nh; ++hd) {
    int b, h, rs;
    ag_head<MEAN>(z, hd, H, b, h);
    const size_t bh = (size_t)b * H + h;
    const size_t base = head_rows(0, b, h, H, N, dh, G::dp_const ? G::dp_const : DP, rs);
    G g;
    g.head(Q + base, K + base, V + base, dO, b, h, H, N, dh, rs, q0 + li, hh, want_p);
    float L[16];   // the lse term of this lane's 16 query rows
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = q0 + ctile_row(i, hh);
      L[i] = (want_p && row < N) ? G::lse_term(lse[bh * (size_t)N + row]) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kb = k0 + 32 * j;
      if (kb < N) {   // wave-uniform
        f32x16 X = g.dprobs(kb + li, N, hh);
        if (want_p) {
          const f32x16 S = g.scores(kb + li, N, hh);
#pragma unroll
          for (int i = 0; i < 16; ++i) X[i] = ag_combine(kind, G::prob(S[i], c, L[i]), X[i]);
        }
        if constexpr (MEAN) {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[j][i] += X[i];
        } else {
          ag_store(out, zbase, X, q0, hh, kb + li, N);
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
        ag_store(out, zbase, acc[j], q0, hh, kb + li, N);
      }
    }
  }
}

// strict fp32: one thread per output element (key on the lane, 4 query rows per workgroup), one FMA chain per product
template <bool MEAN>
__global__ __launch_bounds__(256) void attn_grad_probs_ref_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                                  const float* __restrict__ V,
                                                                  const float* __restrict__ dO,
                                                                  const float* __restrict__ lse, float* __restrict__ out,
                                                                  int H, int N, int dh, int DP, int nqt, int nkt,
                                                                  float scale, float heads, int kind) {
  int z, qt, kt;
  ag_tile(nqt, nkt, z, qt, kt);
  const int row = qt * 4 + (int)(threadIdx.x >> 6), col = kt * 64 + (int)(threadIdx.x & 63);
  if (row >= N || col >= N) return;
  const int nh = MEAN ? H : 1;
  float acc = 0.f;
  for (int hd = 0; hd < nh; ++hd) {
    int b, h, rs;
    ag_head<MEAN>(z, hd, H, b, h);
    const size_t bh = (size_t)b * H + h;
    const size_t base = head_rows(0, b, h, H, N, dh, DP, rs);
    const float* gr = dO + ((size_t)b * N + row) * ((size_t)H * dh) + (size_t)h * dh;
    const float* vr = V + base + (size_t)col * rs;
    float dp = 0.f, p = 0.f;
    for (int d = 0; d < dh; ++d) dp = fmaf(gr[d], vr[d], dp);
    if (kind != SGL_ATTN_GRAD_DP) {
      const float* qr = Q + base + (size_t)row * rs;
      const float* kr = K + base + (size_t)col * rs;
      float s = 0.f;
      for (int d = 0; d < dh; ++d) s = fmaf(qr[d], kr[d], s);
      p = expf(s * scale - lse[bh * (size_t)N + row]);
    }
    acc += ag_combine(kind, p, dp);
  }
  if constexpr (MEAN) acc /= heads;
  out[(size_t)z * (size_t)N * (size_t)N + (size_t)row * (size_t)N + (size_t)col] = acc;
}

}  // namespace

bool attn_grad_probs_shape_ok(int dtype, int B, int H, int N, int dh, int DP) {
  if (!attn_shape_ok(dtype, B, H, N, dh, DP, 0, ATTN_PROBS)) return false;
  // 32-bit byte offsets into one image's dO rows (16-bit kernel)
  if (dtype != DT_F32 && dtype != DT_F32_MFMA && (size_t)N * H * dh * 2 >= (1ull << 31)) return false;
  return true;
}

hipError_t attn_grad_probs(const void* q, const void* k, const void* v, const void* dout, const float* lse, float* out,
                           int dtype, int B, int H, int N, int dh, int DP, int kind, int mode, hipStream_t s) {
  if (!attn_grad_probs_shape_ok(dtype, B, H, N, dh, DP)) return hipErrorInvalidValue;
  if (mode != SGL_ATTN_PROBS_FULL && mode != SGL_ATTN_PROBS_HEAD_MEAN) return hipErrorInvalidValue;
  if (kind != SGL_ATTN_GRAD_DP && kind != SGL_ATTN_GRAD_PDP && kind != SGL_ATTN_GRAD_RELEVANCE) return hipErrorInvalidValue;
  const size_t Z = mode ? B : B * H;
  const AttnScales sc = attn_scales(dh);
  const float heads = (float)H;
  auto launch = [&](auto kernel, auto elem, int nqt, int nkt, float c) {
    using E = decltype(elem);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((size_t)nqt * nkt * Z)), dim3(256), 0, s, (const E*)q, (const E*)k,
                       (const E*)v, (const E*)dout, lse, out, H, N, dh, DP, nqt, nkt, c, heads, kind);
    return hipGetLastError();
  };
  const int nt = (N + 127) / 128;
  return with_bool(mode != 0, [&](auto mean) -> hipError_t {
    constexpr bool MEAN = mean.value;
    if (dtype == DT_F32)
      return launch(attn_grad_probs_ref_kernel<MEAN>, 0.f, (N + 3) / 4, (N + 63) / 64, sc.scale);
    if (dtype == DT_F32_MFMA)
      return launch(attn_grad_probs_kernel<GradF32, MEAN>, 0.f, nt, nt, sc.scale);
    if ((dtype != DT_BF16 && dtype != DT_F16) || !attn_aligned16(q, k, v) || !attn_aligned16(dout, nullptr))
      return hipErrorInvalidValue;
    return dispatch_attn(dtype, DP, [&](auto tag) {
      using T = typename decltype(tag)::type;
      return launch(attn_grad_probs_kernel<GradLo<T, decltype(tag)::dp>, MEAN>, T{}, nt, nt, sc.c);
    });
  });
}

}  // namespace sgl
