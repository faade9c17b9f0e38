// Internal launch API shared by the kernel translation units and the C-ABI host code (encoder.hip).
// Every launcher enqueues on the stream it is given, allocates nothing and never synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "siglip_hip.h"

namespace sgl {

enum DType : int {
  DT_F32 = 0,
  DT_BF16 = 1,
  DT_F32_MFMA = 2,   // attention only: fp32 operands on v_mfma_f32_32x32x2_f32
  DT_F16 = 3,        // fp16 operands on the same MFMA kernels as bf16 (fp32 accumulation)
};
static inline size_t dtype_size(int dt) { return (dt == DT_BF16 || dt == DT_F16) ? 2 : 4; }

// Raises Kernel's dynamic-LDS limit to `bytes` on the first call that succeeds (once per kernel instantiation).
template <auto Kernel>
hipError_t set_max_dynamic_lds_once(int bytes) {
  static bool done = false;
  if (done) return hipSuccess;
  const hipError_t e =
      hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done = e == hipSuccess;
  return e;
}

// the box part of every sgl_view check (preprocess.hip, freq_features.hip): a source of the batch, a non-empty box inside it
static inline bool view_box_ok(const sgl_view& r, int B, int Hs, int Ws) {
  return r.src >= 0 && r.src < B && r.x0 >= 0 && r.x0 < r.x1 && r.x1 <= Ws && r.y0 >= 0 && r.y0 < r.y1 && r.y1 <= Hs;
}

// ---- GEMM epilogues (shared by the MFMA kernels and the strict-fp32 generic kernel) ----------------
enum Epi : int {
  EPI_STORE = 0,      // out[T]   = alpha*acc (+bias)
  EPI_BIAS_GELU = 1,  // out[T]   = u = acc+bias ; out2[T] = gelu_tanh(u)
  EPI_RES_F32 = 2,    // out[f32] = res + acc + bias
  EPI_QKV = 3,        // head-major scatter of acc+bias: out[which][B][H][tokens][head_dim_pad]  (T)
  EPI_GELU_BWD = 4,   // out[T]   = acc * gelu_tanh'(aux[row,col])
  EPI_POS_F32 = 5,    // out[f32] = acc + bias + pos[row % pos_rows, col]
  EPI_F32 = 6,        // out[f32] = alpha*acc (+bias) (+out if accumulate) ; atomicAdd when atomic != 0
};

struct EpiParams {
  void* out = nullptr;   int ldo = 0;
  void* out2 = nullptr;  int ldo2 = 0;
  const float* bias = nullptr;
  const float* res = nullptr;  int ldr = 0;
  const void* aux = nullptr;   int ldaux = 0;
  const float* pos = nullptr;  int pos_rows = 1;
  int tokens = 1, heads = 1, head_dim = 8, head_dim_pad = 8, batch = 1;
  float alpha = 1.0f;
  int accumulate = 0;
  int atomic = 0;
  // EPI_GELU_BWD on the MFMA kernels: when non-null, column sums of the fp32 output tile are atomically added here
  // (= the bias gradient of the GEMM whose output gradient is being produced); must be zeroed/initialised by the host
  float* colsum = nullptr;
  // colsum_ld == 0: atomicAdd into colsum[col].  colsum_ld > 0 (deterministic): the workgroup whose tile starts at row m0
  // STORES its column sums at colsum[(m0 / 128) * colsum_ld + col]; the host zeroes the [ceil(M/128)][colsum_ld] buffer
  // first and folds the rows in a fixed order afterwards (reduce_partials)
  int colsum_ld = 0;
  // EPI_BIAS_GELU / EPI_GELU_BWD pair: when set, the forward stores gelu'(u) in `out` instead of the pre-activation u and
  // the backward multiplies by the saved value instead of re-evaluating the derivative (two transcendentals per element
  // less in the backward epilogue, six plain VALU operations more in the forward one); both launches must agree
  int gelu_grad_form = 0;
  // split-K TN GEMM, deterministic form: split s stores its partial tile at out + s*split_stride (plain stores, ldo = N2)
  // instead of atomically adding into the result; reduce_splits() then sums the slabs in a fixed order
  size_t split_stride = 0;
};

// ---- mx.hip: MX-fp8 (e4m3fn elements, E8M0 scale per 32 K-elements) inference kernels -------------------------------
// An MX operand [rows][Kp] is Kp e4m3 bytes per row (Kp % 128 == 0, zero-padded) plus scales [rows][Kp / 32].
// x [M][K] (ldx elements, DT_F32 or DT_BF16) -> q [M][Kp] + sc [M][Kp/32]
hipError_t quantize_mx(const void* x, int x_dtype, int ldx, int M, int K, int Kp, void* q, void* sc, hipStream_t s);
// LayerNorm (fp32 statistics) of x [M][D] straight into an MX operand [M][Kp] (Kp <= 2048)
hipError_t layernorm_fwd_mx(const float* x, const float* gamma, const float* beta, void* q, void* sc, int M, int D, int Kp,
                            float eps, hipStream_t s);
// C = A . B^T on MX operands (A [M][Kp], B [N][Kp]) with epilogue EPI_RES_F32, EPI_QKV (bf16 output) or EPI_BIAS_GELU
// (MX output: p.out [M][p.ldo] bytes, out_sc [M][p.ldo / 32], N % 32 == 0, p.ldo % 128 == 0; p.out2 unused)
hipError_t gemm_nt_mx(const void* A, const void* As, const void* B, const void* Bs, int M, int N, int Kp, int epi,
                      const EpiParams& p, void* out_sc, hipStream_t s);

// ---- layernorm.hip -----------------------------------------------------------------------------------
hipError_t layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_dtype, int ldy,
                         float* mean, float* rstd, int M, int D, float eps, hipStream_t s);
int layernorm_bwd_blocks(int M);
// partial: [nblk][3*D] floats per block: dgamma, dbeta, column sums of the dx this call wrote
hipError_t layernorm_bwd(const void* dy, int dy_dtype, int lddy, const float* x, const float* mean,
                         const float* rstd, const float* gamma, const float* dres, float* dx, void* dx_lp,
                         int lp_dtype, float* partial, int nblk, int M, int D, hipStream_t s);
// out[j] (+)= sum_b partial[b*stride + j], j < n
hipError_t reduce_partials(const float* partial, int nblk, int stride, float* out, int n, int accumulate,
                           hipStream_t s);
// o_k[j] (+)= sum_b partial[b*stride + k*n + j] for k = 0,1,2 in one launch (null outputs skipped)
hipError_t reduce_partials3(const float* partial, int nblk, int stride, float* o0, float* o1, float* o2, int n, int a0,
                            int a1, int a2, hipStream_t s);

// ---- elementwise.hip ---------------------------------------------------------------------------------
hipError_t im2col(const float* pix, int channels_last, void* out, int out_dtype, int B, int H, int W, int P,
                  int Kp, hipStream_t s);
// the adjoint of im2col: d_cols fp32 [B*(H/P)*(W/P)][Kp] (columns >= 3*P*P never read) -> d_pixels fp32 (B,3,H,W), NCHW or
// NHWC storage (channels_last 0 / 1); every pixel is written, the trailing rows / columns no patch covers with zeros
hipError_t col2im(const float* d_cols, int B, int H, int W, int P, int Kp, float* d_pixels, int channels_last,
                  hipStream_t s);
// dst[r][c] (row stride ldd) = cast(src[r][c]) for r < Rp, c < Cp, zero outside src's R x C
hipError_t cast_pad(const float* src, int R, int C, int lds_, void* dst, int dst_dtype, int Rp, int Cp, int ldd,
                    hipStream_t s);
// One launch for all weight shadows of a block: up to 6 matrices (row-major copy [Rp][Cp] with ld ldd and, optionally, the
// transposed copy [Cp][Rp] with ld ldt, both zero padded outside the R x C source) and up to 4 fp32 vectors (copied, zero padded)
struct CastMat {
  const float* src;
  void* dst;
  void* dst_t;
  int R, C, lds, Rp, Cp, ldd, ldt, tiles_c, tile0;
};
struct CastJob {
  CastMat m[6];
  const float* vsrc[4];
  float* vdst[4];
  int vn[4], vnp[4];
  int nmat = 0, nvec = 0, ntiles = 0;
};
void cast_job_add(CastJob& job, const float* src, int R, int C, int lds_, void* dst, int Rp, int Cp, int ldd, void* dst_t,
                  int ldt);
void cast_job_add_vec(CastJob& job, const float* src, int n, float* dst, int np);
hipError_t cast_job_run(const CastJob& job, int dst_dtype, hipStream_t s);
// bf16x3 operand splits (elementwise.hip): Cs = round_up(C, 8); dst holds 3 * R * Cs bf16
hipError_t split3_rows(const float* src, int R, int C, int ld, void* dst, int Cs, int b_side, hipStream_t s);
hipError_t split3_stack(const float* src, int R, int C, int ld, void* dst, int Cs, int b_side, hipStream_t s);
int colsum_chunks(int M);
// out[j] (+)= sum_r in[r][j] for j < n_out (n_out <= N; N, ld multiples of 8; columns up to N are read)
hipError_t colsum(const void* in, int dtype, int ld, int M, int N, int n_out, float* partial /*[chunks][N]*/,
                  float* out, int accumulate, hipStream_t s);
hipError_t batch_sum(const float* in, int B, size_t n, float* out, int accumulate, hipStream_t s);
// out[j] (+)= sum_i v[i] * W[i*cols + j]; scratch: >= 16 * cols floats
hipError_t vecmat_f32(const float* v, const float* W, int rows, int cols, float* scratch, float* out, int accumulate,
                      hipStream_t s);
hipError_t pos_resize(const float* table, int g0, float* out, int gh, int gw, int D, hipStream_t s);
hipError_t pos_resize_bwd(const float* dout, int gh, int gw, float* dtable, int g0, int D, hipStream_t s);
hipError_t copy_f32(const float* src, float* dst, size_t n, hipStream_t s);
hipError_t cast_f32(const float* src, void* dst, int dst_dtype, size_t n, hipStream_t s);
hipError_t add_f32(const float* a, const float* b, float* out, size_t n, hipStream_t s);  // b may be null
// dst[i] (+)= +0 where src[i] is finite, NaN where it is not
hipError_t zero_unless_nonfinite(const float* src, float* dst, int n, int accumulate, hipStream_t s);

// ---- attention_pool.hip ------------------------------------------------------------------------------
// attention-pool (1 query per image): q [H*dh] fp32, K/V head-major [B][H][N][DP]
// One workgroup per (image, head) keeps, in the default 64 KiB LDS window, one fp32 partial per 8-column chunk of every
// token (the region is reused for the output fold, hence its floor of 256 * 8 floats), the N probabilities (backward: the
// N score gradients as well) and 8 floats of reduction scratch.  pool_attn_lds_floats is that size;
// pool_attn_max_tokens the largest N for which it fits: floor(16376 / (DP / 8 + 1)) forward, floor(16376 / (DP / 8 + 2))
// backward (DP 80: 1488 / 1364; DP 64: 1819 / 1637).  The launchers refuse more with hipErrorInvalidValue, and
// encoder.hip's shape checks refuse it first (SGL_ERR_BAD_SHAPE).
static inline size_t pool_attn_lds_floats(int N, int DP, int backward) {
  const size_t part = (size_t)N * (DP / 8) > (size_t)256 * 8 ? (size_t)N * (DP / 8) : (size_t)256 * 8;
  return part + (backward ? 2 : 1) * (size_t)N + 8;
}
static inline int pool_attn_max_tokens(int DP, int backward) {
  // 16384 floats less the 8 of scratch, over the floats one token takes.  The 2048-float floor never decides: at this n
  // the partials alone are n * c >= 16376 * c / (c + 2) - c floats, which is 5457 at c = DP / 8 = 1 and stays above 2048
  // up to c = 14000 (a head dimension of 112000).
  return (int)((64 * 1024 / sizeof(float) - 8) / (size_t)(DP / 8 + (backward ? 2 : 1)));
}
hipError_t pool_attn_fwd(const float* q, const void* K, const void* V, int dtype, void* out /*[B][H*dh]*/,
                         float* probs /*[B][H][N]*/, int B, int H, int N, int dh, int DP, hipStream_t s);
// Ragged batch (attention.hip.h, "ragged addressing"): K/V head-major [H][T][DP], segment s = rows cu[s] .. cu[s+1]-1; one
// workgroup per (segment, head) on the segment's rows, the LDS window sized for max_n (refused above
// pool_attn_max_tokens(DP, 0)).  Per segment the bits of pool_attn_fwd on that segment alone.
hipError_t pool_attn_fwd_varlen(const float* q, const void* K, const void* V, int dtype, void* out /*[S][H*dh]*/,
                                float* probs /*[H][T]*/, const int* cu /*device [S+1]*/, int S, int T, int max_n, int H,
                                int dh, int DP, hipStream_t s);
// cu[0..S] on the device = exclusive prefix sums of the HOST lengths lens[0..S), carried in kernel arguments (no host copy)
hipError_t seg_offsets(const int* lens, int S, int* cu, hipStream_t s);
hipError_t pool_attn_bwd(const float* q, const void* K, const void* V, int dtype, const float* probs,
                         const float* dout /*[B][H*dh] fp32*/, void* dkv /*[B*N][2*H*dh] T*/,
                         float* dq_partial /*[B][H*dh]*/, int B, int H, int N, int dh, int DP, hipStream_t s);

// ---- gemm_f32.hip: strict-mode generic strided GEMM  C[m,n] = sum_k A(m,k)*B(n,k) ---------------------
hipError_t gemm_f32_generic(const float* A, long sam, long sak, const float* B, long sbn, long sbk, int M, int N,
                            int K, int epi, int out_dtype, const EpiParams& p, hipStream_t s);

// ---- gemm_bf16.hip (128x128 tiles), gemm_bf16_v2.hip (256x256 tiles): MFMA kernels ------------------
// NT: C[M,N] = A[M,K] * B[N,K]^T ; A,B bf16 K-contiguous, lda/ldb multiples of 8, K multiple of 8
hipError_t gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi,
                        int out_dtype, const EpiParams& p, hipStream_t s);
// TN: C[N1,N2] (+)= sum_m A[m,n1] * B[m,n2] ; fp32 output via EPI_F32 (accumulate / atomic split-K)
// out[r*ldo + c] (+)= sum_s ws[s*stride + r*N2 + c]   (fixed summation order)
hipError_t reduce_splits(const float* ws, int splits, size_t stride, int N1, int N2, float* out, int ldo, int accumulate,
                         hipStream_t s);
// split_ws (optional device scratch): when given, the splits of the LDS-DMA kernels write private slabs and
// reduce_splits() sums them (bitwise reproducible); the plan (tn_plan) is the best one whose slabs fit it.  Without
// scratch, or with room for no second slab, the splits add into `out` with fp32 atomics.
hipError_t gemm_tn_bf16(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                        const EpiParams& p, hipStream_t s, float* split_ws = nullptr, size_t split_ws_bytes = 0);
// fp16-operand forms of the two (DT_F16): same kernels, tiles and dispatch; 16-bit outputs are fp16 (out_dtype DT_F16)
hipError_t gemm_nt_f16(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                       const EpiParams& p, hipStream_t s);
hipError_t gemm_tn_f16(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                       const EpiParams& p, hipStream_t s, float* split_ws = nullptr, size_t split_ws_bytes = 0);
// The LDS-DMA kernels of gemm_bf16_v2.hip, which the four above send the shapes that fill the chip to; TIn = bf16 or f16
// (instantiated there).  gemm_nt384 takes EPI_STORE and EPI_RES_F32 only, gemm_nt288 EPI_QKV only (hipErrorInvalidValue otherwise); gemm_tn256 /
// gemm_tn384 run `splits` ranges of m_per tokens (EpiParams::split_stride / atomic say where a split's tile goes).
template <typename TIn>
hipError_t gemm_nt256(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                      const EpiParams& p, hipStream_t s);
template <typename TIn>
hipError_t gemm_nt384(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                      const EpiParams& p, hipStream_t s);
// gemm_nt288: EPI_QKV with a 16-bit output only, 256 x 288 tiles of four whole heads.  Refuses (hipErrorInvalidValue) what nt288_takes_qkv does not hold for:
// the kernel's head-major epilogue addresses with these constants instead of EpiParams::head_dim / head_dim_pad.
constexpr int NT288_BN = 288, NT288_HEAD_DIM = 72, NT288_HEAD_DIM_PAD = 80;
inline bool nt288_takes_qkv(int N, const EpiParams& p) {
  return p.head_dim == NT288_HEAD_DIM && p.head_dim_pad == NT288_HEAD_DIM_PAD && p.heads > 0 &&
         N == 3 * p.heads * NT288_HEAD_DIM && N % NT288_BN == 0;   // the last two: heads % 4 == 0, a tile is inside q, k or v
}
template <typename TIn>
hipError_t gemm_nt288(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                      const EpiParams& p, hipStream_t s);
template <typename TIn>
hipError_t gemm_tn256(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int m_per, int splits,
                      const EpiParams& p, hipStream_t s);
template <typename TIn>
hipError_t gemm_tn384(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int m_per, int splits,
                      const EpiParams& p, hipStream_t s);

// Tile and split of a TN GEMM on the LDS-DMA kernels (N1, N2 >= 512, Mred >= 2048).  The launch is one round of at most
// 256 workgroups, one per CU, so its time is the work of one workgroup: tile area x token rows per split.  Among the
// 256 x 256 and 384 x 192 tiles and every split count with tiles x splits <= 256, at least 1024 rows per split and
// (beyond one split) slabs of splits x N1 x N2 floats inside `ws_bytes`, the plan minimises that product; ties go to the
// 256 x 256 tile and to fewer splits.  One split is always allowed, whatever the tile count.  `tile` = 256 / 384
// considers that geometry only.
struct TnPlan {
  int tile, splits, m_per;   // m_per: rows per split, a multiple of 64; `splits` ranges of it cover Mred
};
constexpr TnPlan tn_plan(int Mred, int N1, int N2, size_t ws_bytes, int tile = 0) {
  TnPlan best = {0, 0, 0};
  long best_cost = 0;
  for (int g = 0; g < 2; ++g) {
    const int bm = g ? 384 : 256, bn = g ? 192 : 256, area8 = g ? 9 : 8;   // tile area in eighths of 256 x 256
    if (tile != 0 && tile != bm) continue;
    const int tiles = ((N1 + bm - 1) / bm) * ((N2 + bn - 1) / bn);
    for (int sp = 1; sp == 1 || (tiles * sp <= 256 && Mred / sp >= 1024); ++sp) {
      if (sp > 1 && (size_t)sp * N1 * N2 * sizeof(float) > ws_bytes) break;
      const int m_per = ((Mred + sp - 1) / sp + 63) / 64 * 64;
      const long cost = (long)area8 * m_per;
      if (best.tile == 0 || cost < best_cost) {
        best = {bm, (Mred + m_per - 1) / m_per, m_per};
        best_cost = cost;
      }
    }
  }
  return best;
}
constexpr bool tn_plan_is(int Mred, int N1, int N2, size_t ws_bytes, int tile, int splits) {
  const TnPlan p = tn_plan(Mred, N1, N2, ws_bytes);
  return (tile == 0 || p.tile == tile) && p.splits == splits;
}
// the bench batch's four dW shapes with a scratch that limits no plan (kTnSlabBytes), and the launches whose digests
// tests/test_gemm_pp_digests_gpu.py records (their split boundaries must not move)
constexpr size_t kTnSlabBytes = (size_t)256 * 384 * 192 * 4;   // tiles x splits <= 256 tiles of at most 384 x 192 floats
static_assert(tn_plan_is(93312, 1152, 1152, kTnSlabBytes, 384, 14), "out_proj dW");
static_assert(tn_plan_is(93312, 3456, 1152, kTnSlabBytes, 384, 4), "QKV dW");
static_assert(tn_plan_is(93312, 4304, 1152, kTnSlabBytes, 256, 3), "fc1 dW");
static_assert(tn_plan_is(93312, 1152, 4304, kTnSlabBytes, 256, 3), "fc2 dW");
static_assert(tn_plan_is(4133, 520, 1152, kTnSlabBytes, 0, 4) && tn_plan(4133, 520, 1152, kTnSlabBytes).m_per == 1088, "digest case");
static_assert(tn_plan_is(2048, 512, 512, kTnSlabBytes, 256, 2) && tn_plan(2048, 512, 512, kTnSlabBytes).m_per == 1024, "digest case");

// ---- attention.hip (attention.hip.h: the shape contract, dispatch and addressing its translation units share) ----
// q,k,v: ld_qkv > 0: token-major [B*N][ld_qkv] column blocks (head h of row r at r*ld_qkv + h*dh; the QKV projection's
// plain output, q/k/v = its three D-wide column blocks); ld_qkv == 0: head-major [B][H][N][DP] with zero pad columns.
// out: token-major [B*N][H*dh]; lse: [B][H][N] (natural log units)
hipError_t attn_fwd(const void* q, const void* k, const void* v, int dtype, void* out, float* lse, int B, int H,
                    int N, int dh, int DP, int ld_qkv, hipStream_t s);
// Ragged batch: q,k,v head-major [H][T][DP] (the ld_qkv == 0 layout at B = 1, N = T), segment s = rows cu[s] .. cu[s+1]-1
// (cu: device int32 [S+1], clamped against T and max_n by the kernels); out token-major [T][H*dh]; lse [H][T].  Per segment
// the bits of attn_fwd(B = 1, N = n_s) on that segment alone.  attn_varlen_shape_ok: what attn_fwd_varlen accepts.
bool attn_varlen_shape_ok(int dtype, int S, int T, int max_n, int H, int dh, int DP);
hipError_t attn_fwd_varlen(const void* q, const void* k, const void* v, int dtype, void* out, float* lse, const int* cu,
                           int S, int T, int max_n, int H, int dh, int DP, hipStream_t s);
// dout: token-major [B*N][H*dh] (T); dqkv: token-major [B*N][3*H*dh] (T); delta: scratch of 2*B*H*N floats
hipError_t attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                    const float* lse, int dtype, void* dqkv, float* delta, int B, int H, int N, int dh, int DP,
                    int ld_qkv, hipStream_t s);

// ---- attention_probs.hip -------------------------------------------------------------------------------
// out[b,h,i,j] = exp2(S_ij * c - lse_i * log2e) from head-major q, k [B][H][N][DP] and the forward's lse [B][H][N]: the P
// the backward kernels rebuild.  mode SGL_ATTN_PROBS_FULL: out (B,H,N,N); SGL_ATTN_PROBS_HEAD_MEAN: out (B,N,N), heads
// summed in ascending order in registers.  fp32 out, plain stores only, inputs const.  hipErrorInvalidValue for an unknown
// dtype / mode, a shape attn_probs_shape_ok (= attn_shape_ok of attention.hip.h for the probs pass) refuses or 16-bit
// operands that are not 16-byte aligned.
bool attn_probs_shape_ok(int dtype, int B, int H, int N, int dh, int DP);
hipError_t attn_probs(const void* q, const void* k, const float* lse, float* out, int dtype, int B, int H, int N, int dh,
                      int DP, int mode, hipStream_t s);
// out [B][N] = (sum_h probs[b][h][n]) / H, heads in ascending order (the pooling head's probe map, head mean)
hipError_t probs_head_mean(const float* probs, float* out, int B, int H, int N, hipStream_t s);

// ---- attention_grad_probs.hip ----------------------------------------------------------------------------
// dP[b,h,i,j] = sum_d dout[b,i,h*dh+d] * v[b,h,j,d] (kind SGL_ATTN_GRAD_DP), P * dP (PDP) or its NaN-keeping relu
// (RELEVANCE), P as attn_probs.  q, k, v head-major [B][H][N][DP]; dout token-major [B*N][H*dh] in the operand dtype (what
// attn_bwd takes); modes, output shapes, stores and refusals as attn_probs, plus an unknown kind.  The shape contract is
// attn_probs' and, for 16-bit operands, 32-bit byte offsets into one image's dout rows.
bool attn_grad_probs_shape_ok(int dtype, int B, int H, int N, int dh, int DP);
hipError_t attn_grad_probs(const void* q, const void* k, const void* v, const void* dout, const float* lse, float* out,
                           int dtype, int B, int H, int N, int dh, int DP, int kind, int mode, hipStream_t s);
// attention_pool.hip: the probe row's form.  da[b,h,n] = sum_d dout[b,h*dh+d] * V[b,h,n,d], combined with probs [B][H][N]
// by `kind`; out (B,H,N) or, head mean, (B,N).  Operands as pool_attn_bwd.
hipError_t pool_attn_grad_probs(const void* V, int dtype, const float* probs, const float* dout /*[B][H*dh] fp32*/,
                                float* out, int B, int H, int N, int dh, int DP, int kind, int mode, hipStream_t s);

}  // namespace sgl
