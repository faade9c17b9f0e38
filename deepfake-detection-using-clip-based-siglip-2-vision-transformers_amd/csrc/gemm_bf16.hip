// bf16 MFMA GEMMs for gfx950 (v_mfma_f32_16x16x32_bf16, fp32 accumulate), 64-lane wavefronts.  The same kernels take
// fp16 operands (DT_F16: v_mfma_f32_16x16x32_f16, same fragment layouts) through their operand-type template parameter.
//
//   gemm_nt : C[M,N]  = A[M,K] · B[N,K]ᵀ      forward projections and dX (with pre-transposed weight shadows)
//   gemm_tn : C[N1,N2] (+)= Σ_m A[m,N1]·B[m,N2]   weight gradients dW = dYᵀ·X, reduction over tokens
//
// Tile 128x128, K-step 64, 256 threads = 4 waves in 2x2, each wave 64x64 = 4x4 MFMA tiles (64 acc VGPRs).
// Operands are staged global -> registers (buffer_load_dwordx4, hardware bounds check supplies zeros for the
// M/K tails) -> LDS, double buffered with one barrier per K-step (loads for step t+1 are issued before the
// MFMAs of step t and written to the other buffer after them).
//
// LDS images (no padding; XOR swizzles so every wide read is bank-conflict free on the 64-bank LDS):
//   NT: [row][64 k] = 128-B rows; 16-B chunk c of row r is stored at chunk c ^ (r & 7); fragments are read with
//       ds_read_b128 (lane = row, 8 consecutive k).
//   TN: [m][128 n] = 256-B rows; chunk c of row m is stored at c ^ (2*(m&3) + 8*((m>>3)&1)); fragments are read
//       with ds_read_b64_tr_b16 (hardware transpose: 4 rows x 16 columns -> lane i gets column i), two reads per
//       8-element fragment, so the token (reduction) index becomes the MFMA k index without any transposed copy
//       of the activations in HBM.
// The accumulator tile is transposed through LDS (fp32, row stride 132) so that the fused epilogue (bias, GELU,
// residual, head-major QKV scatter, ...) works on 8 consecutive columns per lane with 16-byte global accesses.
//
// Roofline: MFMA-bound (arithmetic intensity K/2... >> machine balance); algorithmic FLOPs = 2*M*N*K.
#include <stdlib.h>

#include "common.hip.h"
#include "epilogue.hip.h"
#include "kernels.h"

namespace sgl {

constexpr int G_BM = 128, G_BN = 128, G_BK = 64;
constexpr int G_STAGE = (G_BM + G_BN) * G_BK * 2;  // 32 KiB per stage
constexpr int G_CT_LD = 132;                       // fp32 staging row stride (floats)
constexpr int G_LDS = (2 * G_STAGE > G_BM * G_CT_LD * 4) ? 2 * G_STAGE : G_BM * G_CT_LD * 4;

__device__ __forceinline__ u32x4 ldg128(__amdgpu_buffer_rsrc_t r, uint32_t voff) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
}

// Shared epilogue: acc[i][j] (wave sub-tile) -> LDS fp32 tile -> row-contiguous 8-column chunks -> epi_apply.
template <int EPI, typename TOut>
__device__ __forceinline__ void store_tile(char* smem, f32x4 (&acc)[4][4], int wr, int wc, int lane, int t, int m0,
                                           int n0, int M, int N, const EpiParams& p) {
  float* ct = reinterpret_cast<float*>(smem);
  __syncthreads();  // all waves are done reading the operand stages
  const int g = lane >> 4, c16 = lane & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ct[(wr * 64 + i * 16 + g * 4 + r) * G_CT_LD + wc * 64 + j * 16 + c16] = acc[i][j][r];
  __syncthreads();
  if constexpr (EPI == EPI_F32) {
    if (p.atomic) {
      // split-K: fp32 atomics shaped as 256 contiguous bytes per wave instruction (one dword per lane)
      float* outp = reinterpret_cast<float*>(p.out);
      const int w = t >> 6;
#pragma unroll 4
      for (int rr = 0; rr < 32; ++rr) {
        const int row = w + rr * 4;
        const int grow = m0 + row;
        if (grow >= M) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int col = lane + 64 * h;
          if (n0 + col < N) atomicAdd(outp + (size_t)grow * p.ldo + n0 + col, ct[row * G_CT_LD + col] * p.alpha);
        }
      }
      return;
    }
  }
  // fp32 outputs: 4 columns (16 B) per lane so a wave instruction covers two whole 512-B rows;
  // bf16 outputs: 8 columns (16 B) per lane, four 256-B rows per wave instruction
  constexpr int NV = (sizeof(TOut) == 4) ? 4 : 8;
  constexpr int CPR = G_BN / NV;
  float csum[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) csum[j] = 0.f;
#pragma unroll
  for (int q = 0; q < (G_BM * CPR) / 256; ++q) {
    const int c = t + q * 256;
    const int row = c / CPR, col = (c % CPR) * NV;
    const int grow = m0 + row, gcol = n0 + col;
    if (grow < M && gcol < N) {
      float v[NV];
      Vec<float, NV>::ld(ct + row * G_CT_LD + col, v);
      epi_apply<EPI, TOut, NV>(p, grow, gcol, N, v);
      if constexpr (EPI == EPI_GELU_BWD) {
#pragma unroll
        for (int j = 0; j < NV; ++j) csum[j] += v[j];
      }
    }
  }
  if constexpr (EPI == EPI_GELU_BWD) epi_colsum_fold<256, G_BN, NV>(ct, csum, t, m0, n0, N, p);
}

// ------------------------------------------------------------------------------------------------------
// NT
// ------------------------------------------------------------------------------------------------------
template <int EPI, typename TOut, typename TIn>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(const TIn* __restrict__ A, int lda,
                                                         const TIn* __restrict__ B, int ldb, int M, int N, int K,
                                                         EpiParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int tiles_n = (N + G_BN - 1) / G_BN;
  const int tile_m = blockIdx.x / tiles_n, tile_n = blockIdx.x - tile_m * tiles_n;
  const int m0 = tile_m * G_BM, n0 = tile_n * G_BN;
  const int rows_a = (M - m0 < G_BM) ? M - m0 : G_BM;
  const int rows_b = (N - n0 < G_BN) ? N - n0 : G_BN;
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(A + (size_t)m0 * lda, (uint32_t)(((size_t)(rows_a - 1) * lda + K) * 2));
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(B + (size_t)n0 * ldb, (uint32_t)(((size_t)(rows_b - 1) * ldb + K) * 2));

  // staging assignment: 4 chunks of A and 4 of B per thread; chunk = (row, 8 consecutive k)
  const int srow = t >> 3, skc = t & 7;
  uint32_t a_off[4], b_off[4], l_off[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = srow + q * 32;
    a_off[q] = (row < rows_a) ? (uint32_t)(row * lda + skc * 8) * 2u : SGL_OOB;
    b_off[q] = (row < rows_b) ? (uint32_t)(row * ldb + skc * 8) * 2u : SGL_OOB;
    l_off[q] = (uint32_t)(row * 128 + ((skc ^ (row & 7)) << 4));
  }
  // fragment read offsets (k-step s adds (4*s) to the chunk index before the XOR)
  const int frow = lane & 15, fg = lane >> 4;
  uint32_t fa_row[4], fb_row[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    fa_row[i] = (uint32_t)((wr * 64 + i * 16 + frow) * 128);
    fb_row[i] = (uint32_t)(G_BM * 128 + (wc * 64 + i * 16 + frow) * 128);
  }
  const int fsw = frow & 7;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (K + G_BK - 1) / G_BK;
  u32x4 sa[4], sb[4];
  auto load_tile = [&](int kt) {
    const int k0 = kt * G_BK;
    const bool kok = (k0 + skc * 8) < K;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sa[q] = ldg128(ra, kok ? a_off[q] + (uint32_t)k0 * 2u : SGL_OOB);
      sb[q] = ldg128(rb, kok ? b_off[q] + (uint32_t)k0 * 2u : SGL_OOB);
    }
  };
  auto store_stage = [&](int stage) {
    char* base = smem + stage * G_STAGE;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<u32x4*>(base + l_off[q]) = sa[q];
      *reinterpret_cast<u32x4*>(base + G_BM * 128 + l_off[q]) = sb[q];
    }
  };

  load_tile(0);
  store_stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const char* base = smem + cur * G_STAGE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint32_t coff = (uint32_t)(((4 * s + fg) ^ fsw) << 4);
      lo_x8<TIn> af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[i] = *reinterpret_cast<const lo_x8<TIn>*>(base + fa_row[i] + coff);
        bfr[i] = *reinterpret_cast<const lo_x8<TIn>*>(base + fb_row[i] + coff);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = mfma_16x16x32(af[i], bfr[j], acc[i][j]);
    }
    if (kt + 1 < nk) store_stage(cur ^ 1);
    __syncthreads();
  }
  store_tile<EPI, TOut>(smem, acc, wr, wc, lane, t, m0, n0, M, N, p);
}

// ------------------------------------------------------------------------------------------------------
// TN
// ------------------------------------------------------------------------------------------------------
template <typename TIn>
__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(const TIn* __restrict__ A, int lda,
                                                         const TIn* __restrict__ B, int ldb, int Mred, int N1, int N2,
                                                         int m_per_split, EpiParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int tiles2 = (N2 + G_BN - 1) / G_BN;
  const int tile1 = blockIdx.x / tiles2, tile2 = blockIdx.x - tile1 * tiles2;
  const int n1_0 = tile1 * G_BM, n2_0 = tile2 * G_BN;
  const int m_begin = blockIdx.y * m_per_split;
  const int m_end = (m_begin + m_per_split < Mred) ? m_begin + m_per_split : Mred;
  const int rows = m_end - m_begin;  // > 0 by construction
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(A + (size_t)m_begin * lda, (uint32_t)((size_t)rows * lda * 2));
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(B + (size_t)m_begin * ldb, (uint32_t)((size_t)rows * ldb * 2));

  // staging: tile = 64 rows (m) x 128 columns = 16 chunks per row; 4 chunks per thread per operand
  const int srow = t >> 4, scc = t & 15;
  uint32_t a_off[4], b_off[4], l_off[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = srow + q * 16;
    const int ca = n1_0 + scc * 8, cb = n2_0 + scc * 8;
    a_off[q] = (ca < N1) ? (uint32_t)(row * lda + ca) * 2u : SGL_OOB;
    b_off[q] = (cb < N2) ? (uint32_t)(row * ldb + cb) * 2u : SGL_OOB;
    l_off[q] = (uint32_t)(row * 256 + ((scc ^ (2 * (row & 3) + 8 * ((row >> 3) & 1))) << 4));
  }
  // transposed fragment reads: lane (g = lane>>4, q = (lane>>2)&3, pp = lane&3) supplies row 8g+q(+4), cols 4pp..
  const int fg = lane >> 4, fq = (lane >> 2) & 3, fp = lane & 3;
  const uint32_t swz = (uint32_t)(32 * fq + 128 * (fg & 1));
  const uint32_t frow = (uint32_t)((8 * fg + fq) * 256);
  uint32_t fa_col[4], fb_col[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    fa_col[i] = ((uint32_t)(wr * 128 + i * 32 + 8 * fp)) ^ swz;
    fb_col[i] = ((uint32_t)(wc * 128 + i * 32 + 8 * fp)) ^ swz;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (rows + G_BK - 1) / G_BK;
  u32x4 sa[4], sb[4];
  auto load_tile = [&](int kt) {
    const uint32_t r0 = (uint32_t)kt * G_BK;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // rows past m_end fall outside the descriptor and read as zero
      sa[q] = ldg128(ra, a_off[q] == SGL_OOB ? SGL_OOB : a_off[q] + r0 * (uint32_t)lda * 2u);
      sb[q] = ldg128(rb, b_off[q] == SGL_OOB ? SGL_OOB : b_off[q] + r0 * (uint32_t)ldb * 2u);
    }
  };
  constexpr int OPB = G_BK * 256;  // bytes per operand per stage
  auto store_stage = [&](int stage) {
    char* base = smem + stage * G_STAGE;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<u32x4*>(base + l_off[q]) = sa[q];
      *reinterpret_cast<u32x4*>(base + OPB + l_off[q]) = sb[q];
    }
  };

  load_tile(0);
  store_stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const char* base = smem + cur * G_STAGE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const char* ba = base + s * 32 * 256 + frow;
      const char* bb = ba + OPB;
      lo_x8<TIn> af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const lo_x4<TIn> alo = lds_read_tr16<TIn>(ba + fa_col[i]);
        const lo_x4<TIn> ahi = lds_read_tr16<TIn>(ba + 4 * 256 + fa_col[i]);
        const lo_x4<TIn> blo = lds_read_tr16<TIn>(bb + fb_col[i]);
        const lo_x4<TIn> bhi = lds_read_tr16<TIn>(bb + 4 * 256 + fb_col[i]);
        af[i] = __builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7);
        bfr[i] = __builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = mfma_16x16x32(af[i], bfr[j], acc[i][j]);
    }
    if (kt + 1 < nk) store_stage(cur ^ 1);
    __syncthreads();
  }
  EpiParams pq = p;
  if (p.split_stride) pq.out = reinterpret_cast<float*>(p.out) + (size_t)blockIdx.y * p.split_stride;  // private slab
  store_tile<EPI_F32, float>(smem, acc, wr, wc, lane, t, n1_0, n2_0, N1, N2, pq);
}

// ------------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------------
template <int EPI, typename TOut, typename TIn>
static hipError_t launch_nt(const TIn* A, int lda, const TIn* B, int ldb, int M, int N, int K, const EpiParams& p,
                            hipStream_t s) {
  const hipError_t e = set_max_dynamic_lds_once<&gemm_nt_kernel<EPI, TOut, TIn>>(G_LDS);
  if (e != hipSuccess) return e;
  const int tiles = ((M + G_BM - 1) / G_BM) * ((N + G_BN - 1) / G_BN);
  hipLaunchKernelGGL((gemm_nt_kernel<EPI, TOut, TIn>), dim3(tiles), dim3(256), G_LDS, s, A, lda, B, ldb, M, N, K, p);
  return hipGetLastError();
}

template <typename TIn>
static hipError_t gemm_nt_mfma(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi,
                               int out_dtype, const EpiParams& p, hipStream_t s) {
  if (M == 0 || N == 0) return hipSuccess;
  if ((lda % 8) || (ldb % 8) || (K % 8) || K <= 0) return hipErrorInvalidValue;
  if (epi != EPI_F32 && (N % 8)) return hipErrorInvalidValue;
  if ((size_t)M * lda * 2 >= (1ull << 32) || (size_t)N * ldb * 2 >= (1ull << 32)) return hipErrorInvalidValue;
  if (epi == EPI_QKV && M >= (1 << 22)) return hipErrorInvalidValue;   // qkv_split_row (epilogue.hip.h) is exact below that
  if (M >= 2048 && N >= 256) {
    // Outputs whose width is a whole number of 192-column tiles but not of 256-column ones (the encoder's 1152: fc2 and
    // the three plain-store dX GEMMs) take the 384x192 tile, which has no half-empty last column tile: 1,458 tiles of
    // 1.125 x the work instead of 1,825 at the bench batch, same sums bit for bit.  Measured at M = 93,312 it is 6-7 %
    // faster except with the fp32-residual epilogue at K = 1152 (out_proj: 308 against 310 us, inside the run-to-run
    // spread: that launch is bound by its 860 MB of residual traffic, not by tiles), which therefore stays on the 256x256
    // tile like everything else (N = 4352, 768, ..., the QKV scatter of models whose heads are not 72 wide, and the fp32
    // QKV output of the bf16x3 strict mode).
    // The QKV scatter with a 16-bit output, 72-wide heads stored 80 wide and N = 3 heads 72 a multiple of 288 (so400m: N =
    // 3456 = 12 tiles where the 256-wide tile runs 14) takes the 256x288 tile: four whole heads per tile, written head by
    // head in runs of whole 160-byte rows (store_tile_qkv_heads), same sums bit for bit.
    // SGL_NT_TILE=256|384|288 (developer switch, read once) forces one tile for every shape and epilogue it supports;
    // under 288 a QKV scatter that tile cannot take is refused, not sent elsewhere.
    static const int tile_env = getenv("SGL_NT_TILE") ? atoi(getenv("SGL_NT_TILE")) : 0;
    if (epi == EPI_QKV && out_dtype == (std::is_same<TIn, f16>::value ? DT_F16 : DT_BF16)) {   // as dispatch_epilogue
      const bool can288 = nt288_takes_qkv(N, p);
      if (tile_env == 288 && !can288) return hipErrorInvalidValue;
      if (can288 && (tile_env == 288 || tile_env == 0)) return gemm_nt288<TIn>(A, lda, B, ldb, M, N, K, epi, out_dtype, p, s);
    }
    const bool can384 = epi == EPI_STORE || epi == EPI_RES_F32;
    const bool pays384 = N % 192 == 0 && N % 256 != 0 && (epi == EPI_STORE || K >= 2048);
    const bool want384 = tile_env == 384 || (tile_env != 256 && pays384);
    if (can384 && want384) return gemm_nt384<TIn>(A, lda, B, ldb, M, N, K, epi, out_dtype, p, s);
    return gemm_nt256<TIn>(A, lda, B, ldb, M, N, K, epi, out_dtype, p, s);
  }
  return dispatch_epilogue<TIn>(epi, out_dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch_nt<T::epi, typename T::out, TIn>((const TIn*)A, lda, (const TIn*)B, ldb, M, N, K, p, s);
  });
}
hipError_t gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                        const EpiParams& p, hipStream_t s) {
  return gemm_nt_mfma<bf16>(A, lda, B, ldb, M, N, K, epi, out_dtype, p, s);
}
hipError_t gemm_nt_f16(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                       const EpiParams& p, hipStream_t s) {
  return gemm_nt_mfma<f16>(A, lda, B, ldb, M, N, K, epi, out_dtype, p, s);
}

// whether a TN output with these parameters can be written as private slabs and summed by reduce_splits()
static bool tn_slabs_ok(const EpiParams& p, int N2, const float* split_ws) {
  return p.alpha == 1.0f && !p.bias && (N2 % 4 == 0) && (p.ldo % 4 == 0) &&
         ((((uintptr_t)p.out) | ((uintptr_t)split_ws)) & 15) == 0;
}

// Split the token reduction of a TN GEMM into `splits` ranges of m_per rows (m_per a multiple of G_BK) and run
// launch(m_per, splits, params).  With a workspace that holds every split's slab the splits store private slabs and
// reduce_splits() sums them in a fixed order (deterministic, and ~4x cheaper than the atomic epilogue); otherwise they
// add into the zeroed (or accumulated-into) output with fp32 atomics.
template <typename Launch>
static hipError_t tn_split_k(int Mred, int N1, int N2, int splits, const EpiParams& p_, hipStream_t s, float* split_ws,
                             size_t split_ws_bytes, Launch&& launch) {
  EpiParams p = p_;
  float* out = reinterpret_cast<float*>(p.out);
  if (splits < 1) splits = 1;
  int m_per = (Mred + splits - 1) / splits;
  m_per = ((m_per + G_BK - 1) / G_BK) * G_BK;
  splits = (Mred + m_per - 1) / m_per;
  if (splits > 1) {
    const size_t slab = (size_t)N1 * N2;
    if (split_ws && (size_t)splits * slab * sizeof(float) <= split_ws_bytes && tn_slabs_ok(p, N2, split_ws)) {
      EpiParams q = p;
      q.out = split_ws;
      q.ldo = N2;
      q.accumulate = 0;
      q.atomic = 0;
      q.split_stride = slab;
      const hipError_t e = launch(m_per, splits, q);
      if (e != hipSuccess) return e;
      return reduce_splits(split_ws, splits, slab, N1, N2, out, p.ldo, p.accumulate, s);
    }
    if (!p.accumulate) {
      const hipError_t e = hipMemset2DAsync(out, (size_t)p.ldo * sizeof(float), 0, (size_t)N2 * sizeof(float), N1, s);
      if (e != hipSuccess) return e;
    }
    p.atomic = 1;
  }
  return launch(m_per, splits, p);
}

template <typename TIn>
static hipError_t gemm_tn_mfma(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                               const EpiParams& p, hipStream_t s, float* split_ws, size_t split_ws_bytes) {
  if (N1 == 0 || N2 == 0) return hipSuccess;
  if ((lda % 8) || (ldb % 8)) return hipErrorInvalidValue;
  if ((size_t)Mred * lda * 2 >= (1ull << 32) || (size_t)Mred * ldb * 2 >= (1ull << 32)) return hipErrorInvalidValue;
  if (Mred <= 0) {
    if (!p.accumulate)
      return hipMemset2DAsync(p.out, (size_t)p.ldo * sizeof(float), 0, (size_t)N2 * sizeof(float), N1, s);
    return hipSuccess;
  }
  if (N1 >= 512 && N2 >= 512 && Mred >= 2048) {
    // One workgroup per CU (128 / 144 KiB of LDS) in a single round: tn_plan (kernels.h) chooses the tile and the split of
    // the token reduction.  The slabs of the plan must fit the scratch; if there is no scratch, the output cannot take
    // slabs (tn_split_k) or not even two slabs fit, the plan is made without that limit and the splits add with atomics.
    // SGL_TN_TILE=256|384 (developer switch, read once) allows one geometry only.
    static const int tile_env = getenv("SGL_TN_TILE") ? atoi(getenv("SGL_TN_TILE")) : 0;
    const int tile = (tile_env == 256 || tile_env == 384) ? tile_env : 0;
    const bool slabs_ok = split_ws && tn_slabs_ok(p, N2, split_ws);
    TnPlan plan = tn_plan(Mred, N1, N2, slabs_ok ? split_ws_bytes : 0, tile);
    if (plan.splits == 1) plan = tn_plan(Mred, N1, N2, ~(size_t)0, tile);
    return tn_split_k(Mred, N1, N2, plan.splits, p, s, split_ws, split_ws_bytes, [&](int m_per, int nsplit, const EpiParams& q) {
      if (plan.tile == 384) return gemm_tn384<TIn>(A, lda, B, ldb, Mred, N1, N2, m_per, nsplit, q, s);
      return gemm_tn256<TIn>(A, lda, B, ldb, Mred, N1, N2, m_per, nsplit, q, s);
    });
  }
  return tn_split_k(Mred, N1, N2, splits, p, s, split_ws, split_ws_bytes, [&](int m_per, int nsplit, const EpiParams& q) {
    const hipError_t e = set_max_dynamic_lds_once<&gemm_tn_kernel<TIn>>(G_LDS);
    if (e != hipSuccess) return e;
    const int tiles = ((N1 + G_BM - 1) / G_BM) * ((N2 + G_BN - 1) / G_BN);
    hipLaunchKernelGGL(gemm_tn_kernel<TIn>, dim3(tiles, nsplit), dim3(256), G_LDS, s, (const TIn*)A, lda, (const TIn*)B,
                       ldb, Mred, N1, N2, m_per, q);
    return hipGetLastError();
  });
}
hipError_t gemm_tn_bf16(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                        const EpiParams& p, hipStream_t s, float* split_ws, size_t split_ws_bytes) {
  return gemm_tn_mfma<bf16>(A, lda, B, ldb, Mred, N1, N2, splits, p, s, split_ws, split_ws_bytes);
}
hipError_t gemm_tn_f16(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                       const EpiParams& p, hipStream_t s, float* split_ws, size_t split_ws_bytes) {
  return gemm_tn_mfma<f16>(A, lda, B, ldb, Mred, N1, N2, splits, p, s, split_ws, split_ws_bytes);
}

}  // namespace sgl
