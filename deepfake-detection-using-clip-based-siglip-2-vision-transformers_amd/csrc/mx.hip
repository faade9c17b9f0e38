// MX-fp8 (OCP MXFP8: e4m3fn elements, one E8M0 scale per 32 K-elements) kernels of the SGL_DTYPE_MXFP8 inference mode
// (gfx950): the quantizer, LayerNorm with MX output, and the NT GEMM on v_mfma_scale_f32_16x16x128_f8f6f4.
//
// Storage: an MX operand [rows][Kp] is Kp e4m3 bytes per row (Kp = round_up(K, 128), the GEMM's K-step) plus a scale
// array [rows][Kp / 32] of E8M0 bytes (scale = 2^(byte - 127)).  Padding columns hold zero bytes and zero scale bytes.
//
// Quantizer (the contract tests/test_mxfp8_host.py pins bit for bit), per 32-block of a row with amax = max |x|:
//   e = smallest integer with amax <= 448 * 2^e, clamped to [-127, 127]   (amax = m 2^k, m in [1,2): k-8 if m <= 1.75
//       else k-7);  scale byte e + 127;  elements x * 2^-e rounded to nearest-even into e4m3fn, subnormals kept
//       (no element saturates: |x * 2^-e| <= 448 by construction).  All-zero block: scale byte 0, zero elements.
//   A block holding an inf or NaN gets scale byte 0xFF (E8M0 NaN) and NaN elements (0x7F), so every GEMM output it
//   feeds is NaN.
#include "common.hip.h"
#include "epilogue.hip.h"
#include "kernels.h"

namespace sgl {

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// scale exponent e (see above) from the bit pattern of amax (non-negative); 128 marks a non-finite block
__device__ __forceinline__ int mx_exponent(uint32_t amax_bits) {
  const int ef = (int)(amax_bits >> 23);
  if (ef >= 255) return 128;
  if (ef == 0) return -127;   // zero or fp32-subnormal amax: k <= -127, so e <= -134 clamps to -127
  const int k = ef - 127;
  const int e = (amax_bits & 0x7fffffu) <= 0x600000u ? k - 8 : k - 7;   // m <= 1.75 <=> mantissa field <= 0.75 * 2^23
  return e < -127 ? -127 : e;
}

// |x| <= 448 (finite): e4m3fn byte, round to nearest even, subnormals (m * 2^-9) kept
__device__ __forceinline__ uint32_t e4m3_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  const uint32_t sign = (u >> 24) & 0x80u;
  const uint32_t a = u & 0x7fffffffu;
  uint32_t q;
  if (a < 0x3c800000u) {   // below 2^-6: subnormal grid m * 2^-9 (m = 8 rounds up to the smallest normal, code 0x08)
    q = (uint32_t)rintf(__uint_as_float(a) * 512.0f);
  } else {                 // normal: keep 3 mantissa bits, RNE on the 20 dropped ones; a carry moves into the exponent
    const uint32_t r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;
    q = r - ((127u - 7u) << 3);
  }
  return sign | q;
}

// 32 values -> 8 little-endian words of e4m3 bytes + the scale byte
__device__ __forceinline__ uint32_t mx_quant32(const float* v, uint32_t* w) {
  uint32_t amax = 0;
#pragma unroll
  for (int j = 0; j < 32; ++j) amax = max(amax, __float_as_uint(v[j]) & 0x7fffffffu);
  const int e = mx_exponent(amax);
  if (e == 128) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = 0x7f7f7f7fu;
    return 0xffu;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint32_t x = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) x |= e4m3_rne(ldexpf(v[4 * j + b], -e)) << (8 * b);
    w[j] = x;
  }
  return (uint32_t)(e + 127);
}

__device__ __forceinline__ void st_mx32(uint8_t* q, const uint32_t* w) {
  uint4* d = reinterpret_cast<uint4*>(q);
  d[0] = make_uint4(w[0], w[1], w[2], w[3]);
  d[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// ---- standalone quantize: x [M][K] (ldx elements) -> q [M][Kp] + sc [M][Kp/32]; one thread per 32-block --------------
template <typename T>
__global__ __launch_bounds__(256) void quantize_mx_kernel(const T* __restrict__ x, int ldx, int M, int K, int Kp,
                                                          uint8_t* __restrict__ q, uint8_t* __restrict__ sc) {
  const int nb = Kp >> 5;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)M * nb) return;
  const int row = (int)(idx / nb), b = (int)(idx - (long)row * nb);
  const T* xr = x + (size_t)row * ldx;
  const int c0 = b * 32;
  float v[32];
  const bool vec = c0 + 32 <= K && (ldx % 8) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (vec) {
#pragma unroll
    for (int j = 0; j < 4; ++j) Vec<T, 8>::ld(xr + c0 + 8 * j, v + 8 * j);
  } else {
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = (c0 + j < K) ? Elem<T>::ld(xr + c0 + j) : 0.f;
  }
  uint32_t w[8];
  const uint32_t s = mx_quant32(v, w);
  st_mx32(q + (size_t)row * Kp + c0, w);
  sc[(size_t)row * nb + b] = (uint8_t)s;
}

// ---- LayerNorm forward with MX output: one wave per row, lane b owns the row's 32-block b (Kp / 32 <= 64) ---------------
// Statistics in fp32 exactly as ln_fwd_kernel (mean, then the centred sum of squares; y = (x - mu) * rs * g + b).
__global__ __launch_bounds__(256) void ln_fwd_mx_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, uint8_t* __restrict__ q,
                                                        uint8_t* __restrict__ sc, int M, int D, int Kp, float eps) {
  const int lane = lane_id();
  const int row = blockIdx.x * 4 + wave_id();
  if (row >= M) return;
  const int c0 = lane * 32;
  const float* xr = x + (size_t)row * D;
  float v[32];
#pragma unroll
  for (int j = 0; j < 4; ++j) {   // D % 8 == 0: 8-column chunks are all in or all out
    if (c0 + 8 * j + 8 <= D) {
      Vec<float, 8>::ld(xr + c0 + 8 * j, v + 8 * j);
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) v[8 * j + t] = 0.f;
    }
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) s += v[j];
  const float invD = 1.0f / (float)D;
  const float mu = wave_sum(s) * invD;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const float d = v[j] - mu;
    ss += (c0 + j < D) ? d * d : 0.f;
  }
  const float rs = 1.0f / sqrtf(wave_sum(ss) * invD + eps);
  if (c0 >= Kp) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (c0 + 8 * j + 8 <= D) {
      float g[8], b[8];
      Vec<float, 8>::ld(gamma + c0 + 8 * j, g);
      Vec<float, 8>::ld(beta + c0 + 8 * j, b);
#pragma unroll
      for (int t = 0; t < 8; ++t) v[8 * j + t] = (v[8 * j + t] - mu) * rs * g[t] + b[t];
    }
  }
  uint32_t w[8];
  const uint32_t e = mx_quant32(v, w);
  st_mx32(q + (size_t)row * Kp + c0, w);
  sc[(size_t)row * (Kp >> 5) + lane] = (uint8_t)e;
}

// ---- NT GEMM on MX operands ---------------------------------------------------------------------------------------------
// C[M,N] = A[M,Kp] . B[N,Kp]^T, both MX-fp8 (row stride Kp bytes, scale stride Kp/32), fp32 accumulation.
// 128x128 output tile, 4 waves in 2x2, each 64x64 = 4x4 v_mfma_scale_f32_16x16x128_f8f6f4 per 128-wide K-step.
// Operand lane map (measured on the hardware with one-hot data and per-lane scales): lane l holds row l&15, its bytes
// 0-15 are K-elements 16g .. 16g+15 and bytes 16-31 are 64+16g .. 64+16g+15 of the K-step (g = l>>4); the scale byte in
// bits 0-7 of lane l's scale operand (op_sel 0) applies to row l&15, K-block g (elements 32g .. 32g+31).  So the 32-block
// of a scale is spread over two lane groups, and one lane's 32 bytes straddle two blocks.
// LDS per stage: A and B tiles as 128 rows x 128 B (16-byte chunk c of row r at chunk c ^ (r & 7): the 16 rows one
// ds_read_b128 touches land in 8 distinct bank groups), then one scale dword per row of A and of B.  Two stages, the
// next K-step's global loads in flight during the current step's MFMAs, one barrier per K-step.
constexpr int MX_TILE = 128;
constexpr int MX_STAGE = 2 * MX_TILE * 128 + 2 * MX_TILE * 4;
constexpr int MX_LDS = 2 * MX_STAGE;

struct MxEpi {
  void* out; int ldo;
  uint8_t* out_sc;            // EPI_BIAS_GELU: scales [M][ldo / 32] of the MX output
  const float* bias;
  const float* res; int ldr;
  int tokens, heads, head_dim, head_dim_pad, batch;
};

template <int EPI>
__global__ __launch_bounds__(256) void gemm_nt_mx_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ As,
                                                         const uint8_t* __restrict__ B, const uint8_t* __restrict__ Bs,
                                                         int M, int N, int Kp, MxEpi p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t mx_smem[];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int m0 = blockIdx.y * MX_TILE, n0 = blockIdx.x * MX_TILE;
  const int nks = Kp >> 7, ldsc = Kp >> 5;

  uint4 ga[4], gb[4];
  uint32_t gs = 0;
  auto load = [&](int ks) {
    const size_t k0 = (size_t)ks * 128;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = t + 256 * i, r = c >> 3, ch = c & 7;
      ga[i] = (m0 + r < M) ? *reinterpret_cast<const uint4*>(A + (size_t)(m0 + r) * Kp + k0 + ch * 16) : make_uint4(0, 0, 0, 0);
      gb[i] = (n0 + r < N) ? *reinterpret_cast<const uint4*>(B + (size_t)(n0 + r) * Kp + k0 + ch * 16) : make_uint4(0, 0, 0, 0);
    }
    if (t < 128) gs = (m0 + t < M) ? *reinterpret_cast<const uint32_t*>(As + (size_t)(m0 + t) * ldsc + ks * 4) : 0u;
    else gs = (n0 + t - 128 < N) ? *reinterpret_cast<const uint32_t*>(Bs + (size_t)(n0 + t - 128) * ldsc + ks * 4) : 0u;
  };
  auto store = [&](int stage) {
    uint8_t* base = mx_smem + stage * MX_STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = t + 256 * i, r = c >> 3, ch = c & 7;
      const int off = r * 128 + ((ch ^ (r & 7)) << 4);
      *reinterpret_cast<uint4*>(base + off) = ga[i];
      *reinterpret_cast<uint4*>(base + MX_TILE * 128 + off) = gb[i];
    }
    reinterpret_cast<uint32_t*>(base + 2 * MX_TILE * 128)[t] = gs;   // A scales rows 0..127, then B scales
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  load(0);
  store(0);
  __syncthreads();
  const int g = lane >> 4, rl = lane & 15;
  for (int ks = 0; ks < nks; ++ks) {
    if (ks + 1 < nks) load(ks + 1);
    const uint8_t* base = mx_smem + (ks & 1) * MX_STAGE;
    const uint32_t* sbase = reinterpret_cast<const uint32_t*>(base + 2 * MX_TILE * 128);
    i32x8 fa[4], fb[4];
    int sa[4], sb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ra = 64 * wr + 16 * i + rl, rb = 64 * wc + 16 * i + rl;
      const uint4 a0 = *reinterpret_cast<const uint4*>(base + ra * 128 + ((g ^ (ra & 7)) << 4));
      const uint4 a1 = *reinterpret_cast<const uint4*>(base + ra * 128 + (((g + 4) ^ (ra & 7)) << 4));
      const uint4 b0 = *reinterpret_cast<const uint4*>(base + MX_TILE * 128 + rb * 128 + ((g ^ (rb & 7)) << 4));
      const uint4 b1 = *reinterpret_cast<const uint4*>(base + MX_TILE * 128 + rb * 128 + (((g + 4) ^ (rb & 7)) << 4));
      fa[i] = i32x8{(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
      fb[i] = i32x8{(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
      sa[i] = (int)((sbase[ra] >> (8 * g)) & 0xffu);
      sb[i] = (int)((sbase[MX_TILE + rb] >> (8 * g)) & 0xffu);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
    if (ks + 1 < nks) store((ks + 1) & 1);
    __syncthreads();
  }

  // epilogue: acc[i][j][r] is row m0 + 64 wr + 16 i + 4 g + r, column n0 + 64 wc + 16 j + rl
  if constexpr (EPI == EPI_BIAS_GELU) {
    // MX output (N % 32 == 0): a 32-block is subtiles 2h, 2h+1 of one row, i.e. 16 lanes x 2 registers
    uint8_t* q = reinterpret_cast<uint8_t*>(p.out);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + 64 * wr + 16 * i + 4 * g + r;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int col = n0 + 64 * wc + 32 * h + rl;
          float v0 = 0.f, v1 = 0.f;
          if (col < N) v0 = gelu_tanh(acc[i][2 * h][r] + p.bias[col]);
          if (col + 16 < N) v1 = gelu_tanh(acc[i][2 * h + 1][r] + p.bias[col + 16]);
          uint32_t am = max(__float_as_uint(v0) & 0x7fffffffu, __float_as_uint(v1) & 0x7fffffffu);
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
          const int e = mx_exponent(am);
          uint32_t q0, q1;
          if (e == 128) {
            q0 = q1 = 0x7fu;
          } else {
            q0 = e4m3_rne(ldexpf(v0, -e));
            q1 = e4m3_rne(ldexpf(v1, -e));
          }
          if (row < M && col < N) {
            q[(size_t)row * p.ldo + col] = (uint8_t)q0;
            q[(size_t)row * p.ldo + col + 16] = (uint8_t)q1;
            if (rl == 0) p.out_sc[(size_t)row * (p.ldo >> 5) + (col >> 5)] = (uint8_t)(e == 128 ? 0xff : e + 127);
          }
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = n0 + 64 * wc + 16 * j + rl;
        if (col >= N) continue;
        const float b = p.bias[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + 64 * wr + 16 * i + 4 * g + r;
          if (row >= M) continue;
          if constexpr (EPI == EPI_RES_F32) {
            float* o = reinterpret_cast<float*>(p.out) + (size_t)row * p.ldo + col;
            *o = p.res[(size_t)row * p.ldr + col] + (acc[i][j][r] + b);
          } else {   // EPI_QKV: bf16 head-major scatter [3][B][H][tokens][head_dim_pad], pad columns zeroed
            const int dm = p.heads * p.head_dim;
            const int which = col / dm, hc = col - which * dm, hh = hc / p.head_dim, d = hc - hh * p.head_dim;
            const int bi = row / p.tokens, n = row - bi * p.tokens;
            bf16* dst = reinterpret_cast<bf16*>(p.out) +
                        ((((size_t)which * p.batch + bi) * p.heads + hh) * p.tokens + n) * p.head_dim_pad + d;
            *dst = (bf16)(acc[i][j][r] + b);
            if (d + 1 == p.head_dim)
              for (int z = 1; z < p.head_dim_pad - d; ++z) dst[z] = (bf16)0.f;
          }
        }
      }
  }
}

template <typename T>
hipError_t quantize_launch(const T* x, int ldx, int M, int K, int Kp, uint8_t* q, uint8_t* sc, hipStream_t s) {
  const long n = (long)M * (Kp >> 5);
  quantize_mx_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(x, ldx, M, K, Kp, q, sc);
  return hipGetLastError();
}

template <int EPI>
hipError_t gemm_mx_launch(const uint8_t* A, const uint8_t* As, const uint8_t* B, const uint8_t* Bs, int M, int N, int Kp,
                          const MxEpi& p, hipStream_t s) {
  hipError_t e = set_max_dynamic_lds_once<gemm_nt_mx_kernel<EPI>>(MX_LDS);
  if (e != hipSuccess) return e;
  dim3 grid((N + MX_TILE - 1) / MX_TILE, (M + MX_TILE - 1) / MX_TILE);
  gemm_nt_mx_kernel<EPI><<<grid, 256, MX_LDS, s>>>(A, As, B, Bs, M, N, Kp, p);
  return hipGetLastError();
}

}  // namespace

hipError_t quantize_mx(const void* x, int x_dtype, int ldx, int M, int K, int Kp, void* q, void* sc, hipStream_t s) {
  if (Kp % 128 || K > Kp || K < 0 || ldx < K) return hipErrorInvalidValue;
  if (M == 0 || Kp == 0) return hipSuccess;
  if (x_dtype == DT_BF16)
    return quantize_launch((const bf16*)x, ldx, M, K, Kp, (uint8_t*)q, (uint8_t*)sc, s);
  if (x_dtype == DT_F32)
    return quantize_launch((const float*)x, ldx, M, K, Kp, (uint8_t*)q, (uint8_t*)sc, s);
  return hipErrorInvalidValue;
}

hipError_t layernorm_fwd_mx(const float* x, const float* gamma, const float* beta, void* q, void* sc, int M, int D, int Kp,
                            float eps, hipStream_t s) {
  if (D % 8 || Kp % 128 || D > Kp || Kp > 64 * 32) return hipErrorInvalidValue;
  if (M == 0) return hipSuccess;
  ln_fwd_mx_kernel<<<(M + 3) / 4, 256, 0, s>>>(x, gamma, beta, (uint8_t*)q, (uint8_t*)sc, M, D, Kp, eps);
  return hipGetLastError();
}

hipError_t gemm_nt_mx(const void* A, const void* As, const void* B, const void* Bs, int M, int N, int Kp, int epi,
                      const EpiParams& ep, void* out_sc, hipStream_t s) {
  if (Kp <= 0 || Kp % 128 || M < 0 || N < 0 || !ep.bias) return hipErrorInvalidValue;
  if (M == 0 || N == 0) return hipSuccess;
  MxEpi p{ep.out, ep.ldo, (uint8_t*)out_sc, ep.bias, ep.res, ep.ldr, ep.tokens, ep.heads, ep.head_dim, ep.head_dim_pad,
          ep.batch};
  const uint8_t *a = (const uint8_t*)A, *as = (const uint8_t*)As, *b = (const uint8_t*)B, *bs = (const uint8_t*)Bs;
  switch (epi) {
    case EPI_RES_F32:
      if (!ep.res) return hipErrorInvalidValue;
      return gemm_mx_launch<EPI_RES_F32>(a, as, b, bs, M, N, Kp, p, s);
    case EPI_QKV:
      if (ep.head_dim <= 0 || ep.tokens <= 0 || N % (ep.heads * ep.head_dim)) return hipErrorInvalidValue;
      return gemm_mx_launch<EPI_QKV>(a, as, b, bs, M, N, Kp, p, s);
    case EPI_BIAS_GELU:
      if (N % 32 || ep.ldo % 128 || ep.ldo < N || !out_sc) return hipErrorInvalidValue;
      return gemm_mx_launch<EPI_BIAS_GELU>(a, as, b, bs, M, N, Kp, p, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace sgl
