// Host side of libsiglip_hip.so: the C ABI of include/siglip_hip.h.  Orchestrates the hand-written gfx950
// kernels into the SigLIP-2 vision encoder forward / backward:
//   embeddings   TF:models/siglip/modeling_siglip.py:175-185      (im2col + GEMM, bias + position fused)
//   27x block    TF:...:335-356   x += out_proj(attn(qkv(LN1 x)));  x += fc2(gelu_tanh(fc1(LN2 x)))
//   post LN      TF:...:612        pooling head  TF:...:633-643
// The residual stream, LayerNorm statistics and softmax run in fp32 in every compute mode; GEMM / attention
// operands are bf16 or fp16 (MFMA) or fp32 (strict); the MX-fp8 inference mode (SGL_DTYPE_MXFP8) is the bf16 mode with the
// four projection GEMMs of every block on MX-fp8 operands (mx.hip).  The ctx owns no device memory: every buffer is the
// caller's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "kernels.h"
#include "siglip_hip.h"

using namespace sgl;

namespace {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline char* at(void* base, size_t off) { return reinterpret_cast<char*>(base) + off; }
inline const char* at(const void* base, size_t off) { return reinterpret_cast<const char*>(base) + off; }
// 16-bit MFMA compute modes (bf16, fp16): the same kernels and buffer layouts, only the operand type differs
inline bool mfma16(int dt) { return dt == DT_BF16 || dt == DT_F16; }
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

struct Bump {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += align256(bytes);
    return o;
  }
};

struct ShadowLayer {
  size_t wqkv, wqkv_t, wo, wo_t, w1, w1_t, w2, w2_t, bqkv, b1;
  size_t wqkv_s, wo_s, w1_s, w2_s;   // MX mode: E8M0 scales of the MX matrices at wqkv / wo / w1 / w2 (no transposes)
};

}  // namespace

struct sgl_ctx {
  sgl_config cfg;
  int D, I, Ip, L, H, dh, DP, P, K0, Kp, g0, dt;
  size_t es;  // element size of the compute dtype
  int split = 0;   // SGL_DTYPE_BF16X3: dt == DT_F32 everywhere, GEMMs through the bf16x3 operand split
  int mx = 0;      // SGL_DTYPE_MXFP8: dt == DT_BF16 everywhere except the block GEMMs, which read MX-fp8 operands
  int Dp = 0;      // MX mode: K padding of the D-wide operands, round_up(D, 128) (the MX GEMM's K-step)
  int recompute = 0;   // SGL_RECOMPUTE_BLOCKS: training keeps no per-block activations; sgl_backward_layer* recomputes them
  int last_hip = 0;   // the only member written after sgl_create_ex
  // shadow arena layout (config-only)
  size_t sh_wpatch = 0;
  std::vector<ShadowLayer> sh_layers;
  size_t sh_hwkv = 0, sh_hwkv_t = 0, sh_hwo = 0, sh_hwo_t = 0, sh_hw1 = 0, sh_hw1_t = 0, sh_hw2 = 0, sh_hw2_t = 0,
         sh_hb1 = 0;
  size_t sh_total = 0;
};

namespace {

constexpr int kMaxLayers = 128;

// Slabs of the split-K dW GEMMs: splits * N1 * N2 * 4 bytes.  64 MiB holds every plan of the 256x256 tile (tiles*splits <=
// 256 tiles of 256x256 floats); tn_plan (kernels.h) takes the best plan whose slabs fit, which on the 384x192 tile is 12
// splits instead of 14 for out_proj dW at the bench batch (14 slabs of 1152 x 1152 are 71 MiB).  The size is part of what
// sgl_query_sizes reports and stays as it is.
constexpr size_t kSplitWsBytes = (size_t)256 * 256 * 256 * 4;
static_assert(tn_plan_is(93312, 1152, 1152, kSplitWsBytes, 384, 12), "out_proj dW in the encoder's workspace");
static_assert(tn_plan_is(93312, 3456, 1152, kSplitWsBytes, 384, 4), "QKV dW in the encoder's workspace");
// tests/test_nonfinite_gpu.py holds the scratch-less 2048 x 512 x 512 route to a float64 bound, not to bits, because its
// splits add with fp32 atomics: that rests on the plan splitting this shape
static_assert(tn_plan(2048, 512, 512, ~(size_t)0).splits > 1, "2048 x 512 x 512 dW without scratch: more than one split");

// one of q / k / v of a whole batch, head-major [B][H][N][DP]
inline size_t head_bytes(const sgl_ctx* c, int B, int N) { return (size_t)B * c->H * N * c->DP * c->es; }

// Per-call activation / workspace layout (pure function of ctx, B, grid, train).
struct Layout {
  int B = 0, gh = 0, gw = 0, N = 0, M = 0;
  int PB = 0;   // rows of the pooling head's per-image buffers: B, or the S segments of a ragged batch
  bool train = false;
  // activation region ("saved" when training, a slice of ws otherwise)
  size_t a_im2col = 0, a_pos = 0;
  size_t a_layer0 = 0, a_layer_stride = 0;
  size_t r_stats1 = 0, r_h1 = 0, r_qkv = 0, r_attn = 0, r_lse = 0, r_xmid = 0, r_stats2 = 0, r_h2 = 0, r_u = 0, r_a = 0,
         r_attq = 0;  // relative to a layer base
  size_t a_pstats = 0, a_lastlp = 0, a_kvh = 0, a_qp = 0, a_probs = 0, a_ao = 0, a_h0 = 0, a_hstats = 0, a_hl = 0, a_hu = 0,
         a_ha = 0;
  size_t a_spa = 0, a_spb = 0, w_spa = 0, w_spb = 0;   // bf16x3 split operands (forward: in act; backward: in ws)
  size_t a_cu = 0;   // ragged batch only: the device table cu, int32 [S + 1], last in the activation region
  size_t act_total = 0;
  // backward scratch (ws): all zero unless training
  size_t w_dx = 0, w_g = 0, w_du = 0, w_dh = 0, w_dqkv = 0, w_delta = 0, w_splitws = 0, w_lnpart = 0, w_cspart = 0,
         w_dlast = 0, w_gsum = 0, w_csum = 0;
  size_t w_hg = 0, w_hdu = 0, w_hdh = 0, w_hdao = 0, w_hdqpart = 0, w_hdqp = 0, w_hdh0 = 0;
  size_t ws_bwd_total = 0;
  size_t saved_total = 0, ws_total = 0, ws_act_off = 0;
  // recompute context, training: ONE block region in ws (w_blk) that the forward and every backward block reuse; no
  // per-block region in `saved`, and the forward's bf16x3 split scratch is the backward's (w_spa / w_spb)
  bool rc = false;
  size_t w_blk = 0;

  Layout() = default;
  Layout(const sgl_ctx* c, int B_, int Himg, int Wimg, bool train_) {
    gh = Himg / c->P;
    gw = Wimg / c->P;
    init(c, B_, gh * gw, B_, train_, 0);
  }
  // A ragged inference batch of S images, T tokens in all: the layout of (B = 1, N = T) with S rows in the pooling head's
  // per-image buffers, and cu behind it.  For S = 1 it is the fixed inference layout of that image plus the 256 bytes of cu.
  static Layout ragged(const sgl_ctx* c, int T, int S) {
    Layout l;
    l.init(c, 1, T, S, false, S + 1);
    return l;
  }

 private:
  void init(const sgl_ctx* c, int B_, int N_, int PB_, bool train_, int cu_entries) {
    B = B_;
    PB = PB_;
    train = train_;
    rc = train && c->recompute;
    N = N_;
    M = B * N;
    const size_t es = c->es, D = c->D, Ip = c->Ip, Mz = (size_t)M;
    Bump a;
    a_im2col = a.take(Mz * c->Kp * es);
    a_pos = a.take((size_t)N * D * 4);
    Bump r;
    // MX mode (inference only): r_h1 / r_h2 / r_a hold MX operands (bytes, then their scales), r_attq the quantized
    // attention output; r_u is never written
    const size_t Dp = c->Dp;
    const bool mx = c->mx;
    r_stats1 = r.take(Mz * 2 * 4);
    r_h1 = r.take(mx ? Mz * Dp + Mz * Dp / 32 : Mz * D * es);
    r_qkv = r.take(3 * head_bytes(c, B, N));
    r_attn = r.take(Mz * D * es);
    r_lse = r.take((size_t)B * c->H * N * 4);
    r_xmid = r.take(Mz * D * 4);
    r_stats2 = r.take(Mz * 2 * 4);
    r_h2 = r.take(mx ? Mz * Dp + Mz * Dp / 32 : Mz * D * es);
    r_u = r.take(mx ? 0 : Mz * Ip * es);
    r_a = r.take(mx ? Mz * Ip + Mz * Ip / 32 : Mz * Ip * es);
    r_attq = r.take(mx ? Mz * Dp + Mz * Dp / 32 : 0);
    a_layer_stride = (train && !rc) ? r.off : 0;
    a_layer0 = a.take(rc ? 0 : train ? r.off * (size_t)c->L : r.off);
    a_pstats = a.take(Mz * 2 * 4);
    a_lastlp = a.take(Mz * D * es);
    a_kvh = a.take(2 * head_bytes(c, B, N));
    a_qp = a.take(D * 4);
    a_probs = a.take((size_t)B * c->H * N * 4);
    a_ao = a.take((size_t)PB * D * es);
    a_h0 = a.take((size_t)PB * D * 4);
    a_hstats = a.take((size_t)PB * 2 * 4);
    a_hl = a.take((size_t)PB * D * es);
    a_hu = a.take((size_t)PB * Ip * es);
    a_ha = a.take((size_t)PB * Ip * es);
    // widest GEMM operand: [rows, W] with rows <= max(M, W) on the activation side, [W, max(D, Kp)] on the weight side
    const size_t widest = std::max(Ip, 3 * D), Kp = (size_t)c->Kp;
    const size_t Wd = (size_t)round_up((int)std::max(widest, Kp), 8);
    const size_t sp_act = 3 * std::max(Mz, (size_t)PB) * Wd * 2;
    const size_t sp_wgt = 3 * Wd * (size_t)round_up((int)std::max(D, Kp), 8) * 2;
    const size_t sp_bytes = std::max(sp_act, sp_wgt);
    if (c->split && !rc) {
      a_spa = a.take(sp_bytes);
      a_spb = a.take(sp_bytes);
    }
    if (cu_entries) a_cu = a.take((size_t)cu_entries * 4);
    act_total = a.off;

    Bump w;
    if (train) {
      w_dx = w.take(Mz * D * 4);
      w_g = w.take(Mz * D * es);
      w_du = w.take(Mz * Ip * es);
      w_dh = w.take(Mz * D * es);
      w_dqkv = w.take(Mz * 3 * D * es);
      w_delta = w.take((size_t)B * c->H * N * 8);   // {lse*log2e, delta*scale} pairs
      w_splitws = w.take(kSplitWsBytes);  // private slabs of the split-K dW GEMMs (deterministic reduction)
      w_lnpart = w.take((size_t)layernorm_bwd_blocks(M) * 3 * D * 4);
      w_gsum = w.take(D * 4);        // column sums of the current d hidden_states (bias grad of the GEMM below)
      w_csum = w.take((size_t)((M + 127) / 128) * widest * 4);   // per-row-tile column sums out of a GEMM epilogue
      w_cspart = w.take((size_t)std::max(colsum_chunks(M), 16) * widest * 4);   // also vecmat_f32's 16 row chunks
      w_dlast = w.take(Mz * D * 4);
      w_hg = w.take((size_t)B * D * es);
      w_hdu = w.take((size_t)B * Ip * es);
      w_hdh = w.take((size_t)B * D * es);
      w_hdao = w.take((size_t)B * D * 4);
      w_hdqpart = w.take((size_t)B * D * 4);
      w_hdqp = w.take(D * 4);
      w_hdh0 = w.take((size_t)B * D * 4);
      if (c->split) {
        w_spa = w.take(sp_bytes);
        w_spb = w.take(sp_bytes);
      }
      if (rc) w_blk = w.take(r.off);
    }
    ws_bwd_total = w.off;
    if (train) {
      saved_total = act_total;
      ws_act_off = 0;
      ws_total = ws_bwd_total;
    } else {
      saved_total = 0;
      ws_act_off = ws_bwd_total;
      ws_total = ws_bwd_total + act_total;
    }
    if (ws_total == 0) ws_total = 256;
  }

 public:
  size_t layer_base(int l) const { return a_layer0 + a_layer_stride * (size_t)l; }
};

#define CK(expr)                        \
  do {                                  \
    hipError_t e_ = (expr);             \
    if (e_ != hipSuccess) {             \
      ctx->last_hip = (int)e_;          \
      return SGL_ERR_HIP;               \
    }                                   \
  } while (0)

#define RET(expr)                 \
  do {                            \
    int r_ = (expr);              \
    if (r_ != SGL_OK) return r_;  \
  } while (0)

// ---- epilogue constructors: one per epilogue the encoder uses; whatever one does not set keeps EpiParams' default -----
// EPI_STORE: out[T] = acc
EpiParams epi_store(void* out, int ldo) {
  EpiParams p;
  p.out = out;
  p.ldo = ldo;
  return p;
}
// EPI_F32: out[f32] = acc (+ bias)
EpiParams epi_f32(float* out, int ldo, const float* bias = nullptr) {
  EpiParams p;
  p.out = out;
  p.ldo = ldo;
  p.bias = bias;
  return p;
}
// EPI_F32: out[f32] (+)= acc
EpiParams epi_f32_acc(float* out, int ldo, int accumulate) {
  EpiParams p;
  p.out = out;
  p.ldo = ldo;
  p.accumulate = accumulate;
  return p;
}
// EPI_RES_F32: out[f32] = res + acc + bias (out and res share the row stride ld)
EpiParams epi_res_f32(float* out, const float* bias, const float* res, int ld) {
  EpiParams p;
  p.out = out;
  p.ldo = ld;
  p.bias = bias;
  p.res = res;
  p.ldr = ld;
  return p;
}
// EPI_POS_F32: out[f32] = acc + bias + pos[row % pos_rows]
EpiParams epi_pos_f32(float* out, int ldo, const float* bias, const float* pos, int pos_rows) {
  EpiParams p;
  p.out = out;
  p.ldo = ldo;
  p.bias = bias;
  p.pos = pos;
  p.pos_rows = pos_rows;
  return p;
}
// EPI_BIAS_GELU: a = gelu(acc + bias); u (nullable: not stored) = the pre-activation, or gelu'(u) when grad_form (the
// EPI_GELU_BWD launch that reads it must agree)
EpiParams epi_bias_gelu(void* u, void* a, int ld, const float* bias, int grad_form) {
  EpiParams p;
  p.out = u;
  p.gelu_grad_form = grad_form;
  p.ldo = ld;
  p.out2 = a;
  p.ldo2 = ld;
  p.bias = bias;
  return p;
}
// EPI_BIAS_GELU of the MX GEMM: gelu(acc + bias) quantized into the MX operand `out` (its scales are a launch argument)
EpiParams epi_bias_gelu_mx(void* out, int ldo, const float* bias) {
  EpiParams p;
  p.out = out;
  p.ldo = ldo;
  p.bias = bias;
  return p;
}
// EPI_GELU_BWD: out = acc * gelu'(u) with u (or gelu'(u) when grad_form) in aux.  colsum (nullable, MFMA kernels only): the
// deterministic per-128-row-tile column sums of the output, [ceil(M / 128)][ld]; the caller zeroes it first and folds it after
EpiParams epi_gelu_bwd(void* out, const void* aux, int ld, int grad_form, float* colsum = nullptr) {
  EpiParams p;
  p.out = out;
  p.ldo = ld;
  p.aux = aux;
  p.ldaux = ld;
  p.gelu_grad_form = grad_form;
  if (colsum) {
    p.colsum = colsum;
    p.colsum_ld = ld;
  }
  return p;
}

// the split-K count of a dW GEMM: enough splits for 512 workgroups, each reducing at least 512 rows, 16 at the most
int tn_splits(int N1, int N2, int rows) {
  const int tiles = ((N1 + 127) / 128) * ((N2 + 127) / 128);
  return std::min({(512 + tiles - 1) / tiles, std::max(rows / 512, 1), 16});
}

// Everything one entry-point call works on, yielded by begin_call() once the arguments have passed their checks and
// handed to every stage.  The ctx is immutable after sgl_create_ex (but for last_hip) and owns no memory; what belongs to
// this call, the bf16x3 split scratch included, is here, so a GEMM cannot be launched on another call's buffers.
struct Call {
  sgl_ctx* ctx = nullptr;   // non-const only because CK records last_hip through it
  Layout lay;
  hipStream_t s = nullptr;
  const void* shadow = nullptr;
  char* act = nullptr;   // activation arena: `saved` (written by the forward only), or its slice of ws at inference
  void* ws = nullptr;
  void* sp_a = nullptr;   // bf16x3: split operands of the GEMM being launched (calls on one ctx are stream-ordered)
  void* sp_b = nullptr;
  // a ragged batch (sgl_forward_ragged): the device table of its S segments and the longest one; NULL on every other call
  const int* cu = nullptr;
  int S = 0, max_n = 0;

  char* wsp(size_t off) const { return at(ws, off); }
  float* wsf(size_t off) const { return reinterpret_cast<float*>(at(ws, off)); }
  float* actf(size_t off) const { return reinterpret_cast<float*>(act + off); }
  const char* sh(size_t off) const { return at(shadow, off); }
  const float* shf(size_t off) const { return reinterpret_cast<const float*>(at(shadow, off)); }
  size_t head_bytes() const { return ::head_bytes(ctx, lay.B, lay.N); }
  // block l's activation region: in the activation arena, or (recompute, training) the one region in ws
  char* block(int l) const { return lay.rc ? wsp(lay.w_blk) : act + lay.layer_base(l); }

  // EPI_QKV: head-major scatter of acc + bias into out[which][B][H][N][DP], geometry of this call
  EpiParams epi_qkv(void* out, const float* bias) const {
    EpiParams p;
    p.out = out;
    p.bias = bias;
    p.tokens = lay.N;
    p.heads = ctx->H;
    p.head_dim = ctx->dh;
    p.head_dim_pad = ctx->DP;
    p.batch = lay.B;
    return p;
  }

  // the block attention of this call on head-major q | k | v: per image, or per segment of a ragged batch
  hipError_t attention(const char* q, int dtype, void* out, float* lse) const {
    const char *k = q + head_bytes(), *v = q + 2 * head_bytes();
    if (cu) return attn_fwd_varlen(q, k, v, dtype, out, lse, cu, S, lay.N, max_n, ctx->H, ctx->dh, ctx->DP, s);
    return attn_fwd(q, k, v, dtype, out, lse, lay.B, ctx->H, lay.N, ctx->dh, ctx->DP, 0, s);
  }
  // the pooling head's probe attention on head-major k | v, likewise
  hipError_t pool_attention(const float* qp, const char* kv, void* out, float* probs) const {
    if (cu)
      return pool_attn_fwd_varlen(qp, kv, kv + head_bytes(), ctx->dt, out, probs, cu, S, lay.N, max_n, ctx->H, ctx->dh,
                                  ctx->DP, s);
    return pool_attn_fwd(qp, kv, kv + head_bytes(), ctx->dt, out, probs, lay.B, ctx->H, lay.N, ctx->dh, ctx->DP, s);
  }

  // C[M,N] = A[M,K] · B[N,K]^T through epilogue epi
  hipError_t gemm_nt(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dt,
                     const EpiParams& p) const {
    if (ctx->dt == DT_BF16) return gemm_nt_bf16(A, lda, B, ldb, M, N, K, epi, out_dt, p, s);
    if (ctx->dt == DT_F16) return gemm_nt_f16(A, lda, B, ldb, M, N, K, epi, out_dt, p, s);
    if (ctx->split && M > 0 && N > 0) {   // bf16x3: one MFMA GEMM over [hi|hi|lo] x [hi|lo|hi], three times the reduction length
      const int Ks = round_up(K, 8);
      hipError_t e = split3_rows((const float*)A, M, K, lda, sp_a, Ks, 0, s);
      if (e != hipSuccess) return e;
      e = split3_rows((const float*)B, N, K, ldb, sp_b, Ks, 1, s);
      if (e != hipSuccess) return e;
      return gemm_nt_bf16(sp_a, 3 * Ks, sp_b, 3 * Ks, M, N, 3 * Ks, epi, out_dt, p, s);
    }
    return gemm_f32_generic((const float*)A, lda, 1, (const float*)B, ldb, 1, M, N, K, epi, out_dt, p, s);
  }

  // dW[N1,N2] (+)= A[:, :N1]^T · B[:, :N2]   (reduction over the Mred rows); split_slabs: the K-splits write the private slabs
  // of w_splitws and are summed in a fixed order (the GEMMs over all M tokens), instead of adding into out
  hipError_t gemm_tn(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, float* out, int ldo,
                     int accumulate, bool split_slabs) const {
    const EpiParams p = epi_f32_acc(out, ldo, accumulate);
    float* slabs = split_slabs ? wsf(lay.w_splitws) : nullptr;
    const size_t slab_bytes = split_slabs ? kSplitWsBytes : 0;
    if (ctx->dt == DT_F16)
      return gemm_tn_f16(A, lda, B, ldb, Mred, N1, N2, tn_splits(N1, N2, Mred), p, s, slabs, slab_bytes);
    if (ctx->dt == DT_BF16)
      return gemm_tn_bf16(A, lda, B, ldb, Mred, N1, N2, tn_splits(N1, N2, Mred), p, s, slabs, slab_bytes);
    if (ctx->split && Mred > 0 && N1 > 0 && N2 > 0) {   // bf16x3: [hi;hi;lo]^T x [hi;lo;hi], reduction over 3*Mred rows
      const int l1 = round_up(N1, 8), l2 = round_up(N2, 8);
      hipError_t e = split3_stack((const float*)A, Mred, N1, lda, sp_a, l1, 0, s);
      if (e != hipSuccess) return e;
      e = split3_stack((const float*)B, Mred, N2, ldb, sp_b, l2, 1, s);
      if (e != hipSuccess) return e;
      return gemm_tn_bf16(sp_a, l1, sp_b, l2, 3 * Mred, N1, N2, tn_splits(N1, N2, 3 * Mred), p, s, slabs, slab_bytes);
    }
    return gemm_f32_generic((const float*)A, 1, lda, (const float*)B, 1, ldb, N1, N2, Mred, EPI_F32, DT_F32, p, s);
  }

  // bias gradient: out[0:n_out] (+)= colsum(in[:, 0:N]); a null out is skipped
  int bias_grad(const void* in, int ld, int M, int N, int n_out, float* out, int accumulate) const {
    if (!out) return SGL_OK;
    CK(colsum(in, ctx->dt, ld, M, N, n_out, wsf(lay.w_cspart), out, accumulate, s));
    return SGL_OK;
  }

  // LayerNorm backward + dgamma/dbeta reduction.  colsum_out (nullable, [D]) = column sums of the dx written, i.e. the
  // bias gradient of the Linear whose output gradient dx is.
  int ln_backward(const void* dy, int dy_dt, const float* x, const float* stats, int rows, const float* gamma,
                  const float* dres, float* dx, void* dx_lp, float* dgamma, float* dbeta, int accumulate,
                  float* colsum_out = nullptr) const {
    const int D = ctx->D;
    const bool want = dgamma || dbeta || colsum_out;
    const int nblk = layernorm_bwd_blocks(rows);
    float* part = wsf(lay.w_lnpart);
    CK(layernorm_bwd(dy, dy_dt, D, x, stats, stats + rows, gamma, dres, dx, dx_lp, ctx->dt, want ? part : nullptr, nblk,
                     rows, D, s));
    CK(reduce_partials3(part, nblk, 3 * D, dgamma, dbeta, colsum_out, D, accumulate, accumulate, 0, s));
    return SGL_OK;
  }
};

// One encoder block of the MX-fp8 mode: x -> xo through xmid, with the four projection GEMMs on MX operands.
//   LN1 -> MX (r_h1) ; QKV GEMM -> bf16 head-major (r_qkv) ; bf16 attention -> r_attn ; quantize -> MX (r_attq) ;
//   out_proj + bias + x -> xmid ; LN2 -> MX (r_h2) ; fc1 + bias, GELU, quantized in the epilogue -> MX (r_a) ;
//   fc2 + bias + xmid -> xo
int mx_block(const Call& c, const sgl_layer_weights& lw, const ShadowLayer& sl, char* lb, const float* x, float* xo) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, Ip = ctx->Ip, Dp = ctx->Dp, M = lay.M;
  const float eps = ctx->cfg.layer_norm_eps;
  const size_t Mz = (size_t)M;
  char* h1 = lb + lay.r_h1;
  char* q = lb + lay.r_qkv;
  char* aq = lb + lay.r_attq;
  float* xmid = reinterpret_cast<float*>(lb + lay.r_xmid);
  char* h2 = lb + lay.r_h2;
  char* ua = lb + lay.r_a;
  CK(layernorm_fwd_mx(x, lw.ln1_w, lw.ln1_b, h1, h1 + Mz * Dp, M, D, Dp, eps, s));
  CK(gemm_nt_mx(h1, h1 + Mz * Dp, c.sh(sl.wqkv), c.sh(sl.wqkv_s), M, 3 * D, Dp, EPI_QKV, c.epi_qkv(q, c.shf(sl.bqkv)),
                nullptr, s));
  CK(c.attention(q, DT_BF16, lb + lay.r_attn, reinterpret_cast<float*>(lb + lay.r_lse)));
  // a 32-block of the attention output straddles heads when head_dim = 72: a pass of its own, not an attention epilogue
  CK(quantize_mx(lb + lay.r_attn, DT_BF16, D, M, D, Dp, aq, aq + Mz * Dp, s));
  CK(gemm_nt_mx(aq, aq + Mz * Dp, c.sh(sl.wo), c.sh(sl.wo_s), M, D, Dp, EPI_RES_F32, epi_res_f32(xmid, lw.o_b, x, D),
                nullptr, s));
  CK(layernorm_fwd_mx(xmid, lw.ln2_w, lw.ln2_b, h2, h2 + Mz * Dp, M, D, Dp, eps, s));
  CK(gemm_nt_mx(h2, h2 + Mz * Dp, c.sh(sl.w1), c.sh(sl.w1_s), M, Ip, Dp, EPI_BIAS_GELU,
                epi_bias_gelu_mx(ua, Ip, c.shf(sl.b1)), ua + Mz * Ip, s));
  CK(gemm_nt_mx(ua, ua + Mz * Ip, c.sh(sl.w2), c.sh(sl.w2_s), M, D, Ip, EPI_RES_F32, epi_res_f32(xo, lw.fc2_b, xmid, D),
                nullptr, s));
  return SGL_OK;
}

// One encoder block of the 16-bit / strict modes up to the MLP's hidden activation: LN1 -> QKV (head-major) -> attention
// -> out_proj + bias + x = xmid -> LN2 -> fc1 + bias, GELU into the block region lb (u = the pre-activation, or gelu'(u)
// in bf16 / fp16 mode, only when want_u).  The training forward and the recompute of sgl_backward_layer* share it, so
// both launch the same kernels on the same shapes and produce the same bits.
int block_to_fc1(const Call& c, const sgl_layer_weights& lw, const ShadowLayer& sl, char* lb, const float* x, bool want_u) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, Ip = ctx->Ip, M = lay.M, dt = ctx->dt;
  const float eps = ctx->cfg.layer_norm_eps;
  float* st1 = reinterpret_cast<float*>(lb + lay.r_stats1);
  float* st2 = reinterpret_cast<float*>(lb + lay.r_stats2);
  char* q = lb + lay.r_qkv;
  float* xmid = reinterpret_cast<float*>(lb + lay.r_xmid);
  CK(layernorm_fwd(x, lw.ln1_w, lw.ln1_b, lb + lay.r_h1, dt, D, st1, st1 + M, M, D, eps, s));
  // head-major scatter [3][B][H][N][DP] in the GEMM epilogue (EPI_QKV).  Round 3 measured the alternative the kernels
  // also support (ld_qkv > 0: plain token-major [M][3D] store, attention gathers each head's 144-byte row segments):
  // QKV GEMM 853 -> 754 us per launch at B = 128, but attention forward +5.8 % and backward +5.9 % (every DMA instruction
  // touches 14 cache lines instead of 8, and K/V are re-read by six workgroups per head and three kernels): +0.75 ms
  // per step net, so the 144-byte granularity is paid once, on the write side.
  CK(c.gemm_nt(lb + lay.r_h1, D, c.sh(sl.wqkv), D, M, 3 * D, D, EPI_QKV, dt, c.epi_qkv(q, c.shf(sl.bqkv))));
  CK(c.attention(q, ctx->split ? DT_F32_MFMA : dt, lb + lay.r_attn, reinterpret_cast<float*>(lb + lay.r_lse)));
  CK(c.gemm_nt(lb + lay.r_attn, D, c.sh(sl.wo), D, M, D, D, EPI_RES_F32, DT_F32, epi_res_f32(xmid, lw.o_b, x, D)));
  CK(layernorm_fwd(xmid, lw.ln2_w, lw.ln2_b, lb + lay.r_h2, dt, D, st2, st2 + M, M, D, eps, s));
  // r_u holds gelu'(u) in bf16 / fp16 mode (the backward only ever needs that)
  CK(c.gemm_nt(lb + lay.r_h2, D, c.sh(sl.w1), D, M, Ip, D, EPI_BIAS_GELU, dt,
               epi_bias_gelu(want_u ? lb + lay.r_u : nullptr, lb + lay.r_a, Ip, c.shf(sl.b1), mfma16(dt))));
  return SGL_OK;
}

// Patch embedding: pixels -> im2col operand (kept in act for the backward) -> GEMM + bias + position table = out
int embed_forward(const Call& c, const sgl_weights* w, const float* pixels, int channels_last, int H, int W, float* out) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, Kp = ctx->Kp, M = lay.M;
  char* cols = c.act + lay.a_im2col;
  if (channels_last == 2) {   // ready patch-major operand (sgl_op_preprocess): keep a copy where backward expects it
    CK(hipMemcpyAsync(cols, pixels, (size_t)M * Kp * ctx->es, hipMemcpyDeviceToDevice, s));
  } else {
    CK(im2col(pixels, channels_last, cols, ctx->dt, lay.B, H, W, ctx->P, Kp, s));
  }
  const float* pos = w->pos;
  if (!(lay.gh == ctx->g0 && lay.gw == ctx->g0)) {
    float* pr = c.actf(lay.a_pos);
    CK(pos_resize(w->pos, ctx->g0, pr, lay.gh, lay.gw, D, s));
    pos = pr;
  }
  CK(c.gemm_nt(cols, Kp, c.sh(ctx->sh_wpatch), Kp, M, D, Kp, EPI_POS_F32, DT_F32,
               epi_pos_f32(out, D, w->patch_b, pos, lay.N)));
  return SGL_OK;
}

// Attention-pool head: pooled = h0 + fc2(gelu(fc1(LN(h0)))), h0 = out_proj(attn(probe · Wq, kv(last_hidden)))
int head_forward(const Call& c, const sgl_weights* w, const float* last_hidden, float* pooled) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, Ip = ctx->Ip, M = lay.M, B = lay.PB, dt = ctx->dt;   // B: pooled rows (images, or segments)
  char* act = c.act;
  char* kv = act + lay.a_kvh;
  float* qp = c.actf(lay.a_qp);
  float* h0 = c.actf(lay.a_h0);
  float* hst = c.actf(lay.a_hstats);
  CK(cast_f32(last_hidden, act + lay.a_lastlp, dt, (size_t)M * D, s));
  CK(c.gemm_nt(act + lay.a_lastlp, D, c.sh(ctx->sh_hwkv), D, M, 2 * D, D, EPI_QKV, dt, c.epi_qkv(kv, w->in_proj_b + D)));
  CK(gemm_f32_generic(w->probe, D, 1, w->in_proj_w, D, 1, 1, D, D, EPI_F32, DT_F32, epi_f32(qp, D, w->in_proj_b), s));
  CK(c.pool_attention(qp, kv, act + lay.a_ao, c.actf(lay.a_probs)));
  CK(c.gemm_nt(act + lay.a_ao, D, c.sh(ctx->sh_hwo), D, B, D, D, EPI_F32, DT_F32, epi_f32(h0, D, w->out_proj_b)));
  CK(layernorm_fwd(h0, w->head_ln_w, w->head_ln_b, act + lay.a_hl, dt, D, hst, hst + B, B, D, ctx->cfg.layer_norm_eps, s));
  // the head keeps the pre-activation u in every mode (gelu_grad_form = 0), unlike the blocks
  CK(c.gemm_nt(act + lay.a_hl, D, c.sh(ctx->sh_hw1), D, B, Ip, D, EPI_BIAS_GELU, dt,
               epi_bias_gelu(act + lay.a_hu, act + lay.a_ha, Ip, c.shf(ctx->sh_hb1), 0)));
  CK(c.gemm_nt(act + lay.a_ha, Ip, c.sh(ctx->sh_hw2), Ip, B, D, Ip, EPI_RES_F32, DT_F32,
               epi_res_f32(pooled, w->head_fc2_b, h0, D)));
  return SGL_OK;
}

// Largest token count M = B * grid a pass accepts, on every context (size audit).  The MFMA GEMM
// dispatchers refuse any operand of 2^32 bytes or more (32-bit buffer-descriptor ranges), so the limit is what keeps the
// widest operand with M rows that the pass hands to gemm_nt / gemm_tn below that:
//   forward   [M][max(Ip, D, Kp)]    a (fc2), h1 / attn / h2 / the head's cast of the last hidden state, im2col
//   training  [M][max(Ip, 3D, Kp)]   the forward's, and u / du, dqkv (dX and dW of the QKV projection)
// three times as wide after the bf16x3 split ([M][3 * round_up(K, 8)] bf16), 4-byte in strict fp32 (gemm_f32_generic has
// no such guard; its limit is the same operand extent, which is what has been audited and is tested).  The EPI_QKV row
// division (qkv_split_row) is exact for rows < 2^22: every context is capped there, the blocks' and the head's K/V scatter
// both use it.  MX-fp8: its own kernels index with size_t and divide exactly, and gemm_nt_mx has no operand guard; what
// bounds it are the bf16 GEMMs it still runs (im2col [M][Kp], the head's [M][D] cast) and the 65 535 row tiles of
// gemm_nt_mx's grid.y.
long max_tokens(const sgl_ctx* c, bool train) {
  const long cap = (1l << 22) - 1;
  long w = c->Ip, row_bytes;
  if ((long)c->D > w) w = c->D;
  if ((long)c->Kp > w) w = c->Kp;
  if (c->mx) {
    row_bytes = 2 * (long)std::max(c->D, c->Kp);
  } else {
    if (train && 3l * c->D > w) w = 3l * c->D;
    row_bytes = c->split ? 3 * (long)round_up((int)w, 8) * 2 : w * (long)c->es;
  }
  long m = ((1l << 32) - 1) / row_bytes;
  if (c->mx && m > 65535l * 128) m = 65535l * 128;
  return m < cap ? m : cap;
}

bool shape_ok(const sgl_ctx* c, int B, int H, int W, bool train = false) {
  if (B <= 0 || H <= 0 || W <= 0) return false;
  if (H < c->P || W < c->P) return false;  // 'valid' conv: trailing pixels beyond gh*P are ignored
  const long N = (long)(H / c->P) * (W / c->P);
  if ((long)B * N > max_tokens(c, train)) return false;
  if (c->cfg.use_head && N > pool_attn_max_tokens(c->DP, 0)) return false;   // the pooling head's LDS window (kernels.h)
  return true;
}

// shape_ok with the training token limit, plus the pooling head's (smaller) backward token limit
bool train_shape_ok(const sgl_ctx* c, int B, int H, int W) {
  if (!shape_ok(c, B, H, W, true)) return false;
  const long N = (long)(H / c->P) * (W / c->P);
  return !(c->cfg.use_head && N > pool_attn_max_tokens(c->DP, 1));
}

// The prologue of every encoder call, after the entry point's own pointer checks (ctx among them) and before anything is
// enqueued: shape, mode, Layout, arena pointers and sizes, then the Call.  A forward trains iff it is given `saved`; a
// plain training forward keeps everything there and leaves the workspace alone, inference and a recompute context's
// training forward (its block region) use ws; a backward needs both arenas.  The order of the checks is the order in
// which a call invalid in several arguments reports them, and differs between the two families as it always has.
enum Pass { FORWARD, BACKWARD };
int begin_call(Call& c, Pass pass, sgl_ctx* ctx, const void* shadow, int B, int H, int W, const void* saved,
               size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream) {
  const bool train = pass == BACKWARD || saved != nullptr;
  if (!(train ? train_shape_ok(ctx, B, H, W) : shape_ok(ctx, B, H, W))) return SGL_ERR_BAD_SHAPE;
  if (train && ctx->mx) return SGL_ERR_UNSUPPORTED;   // the MX-fp8 mode has no backward
  c.lay = Layout(ctx, B, H, W, train);
  const Layout& lay = c.lay;
  if (pass == BACKWARD) {
    if (!saved || !ws) return SGL_ERR_NULL;
    if (saved_bytes < lay.saved_total || ws_bytes < lay.ws_total) return SGL_ERR_WORKSPACE;
  } else {
    const bool needs_ws = !train || lay.rc;
    if (train && saved_bytes < lay.saved_total) return SGL_ERR_WORKSPACE;
    if (needs_ws && !ws) return SGL_ERR_NULL;
    if (needs_ws && ws_bytes < lay.ws_total) return SGL_ERR_WORKSPACE;
  }
  c.ctx = ctx;
  c.s = (hipStream_t)stream;
  c.shadow = shadow;
  c.ws = ws;
  c.act = train ? reinterpret_cast<char*>(const_cast<void*>(saved)) : at(ws, lay.ws_act_off);
  if (ctx->split) {   // forward: in act, or in ws on a recompute context; backward: in ws
    const bool in_ws = pass == BACKWARD || lay.rc;
    c.sp_a = in_ws ? at(ws, lay.w_spa) : c.act + lay.a_spa;
    c.sp_b = in_ws ? at(ws, lay.w_spb) : c.act + lay.a_spb;
  }
  return SGL_OK;
}

}  // namespace

// =======================================================================================================
extern "C" {

int sgl_abi_version(void) { return 3; }

const char* sgl_status_string(int status) {
  switch (status) {
    case SGL_OK: return "ok";
    case SGL_ERR_BAD_SHAPE: return "bad shape";
    case SGL_ERR_UNSUPPORTED: return "unsupported configuration";
    case SGL_ERR_WORKSPACE: return "buffer too small";
    case SGL_ERR_HIP: return "HIP error";
    case SGL_ERR_NULL: return "null pointer";
  }
  return "unknown";
}

sgl_ctx* sgl_create(const sgl_config* cfg) { return sgl_create_ex(cfg, SGL_RECOMPUTE_NONE); }

sgl_ctx* sgl_create_ex(const sgl_config* cfg, int recompute) {
  if (!cfg) return nullptr;
  if (recompute != SGL_RECOMPUTE_NONE && recompute != SGL_RECOMPUTE_BLOCKS) return nullptr;
  if (recompute && cfg->compute_dtype == SGL_DTYPE_MXFP8) return nullptr;   // the MX-fp8 mode never trains
  if (cfg->hidden_size <= 0 || cfg->num_heads <= 0 || cfg->hidden_size % cfg->num_heads) return nullptr;
  const int dh = cfg->hidden_size / cfg->num_heads;
  if (dh % 8 || dh > 96 || cfg->hidden_size % 8 || cfg->hidden_size > 2048) return nullptr;
  if (cfg->intermediate_size <= 0 || cfg->num_layers < 0 || cfg->num_layers > 128 || cfg->patch_size <= 0 ||
      cfg->native_grid <= 0)
    return nullptr;
  if (cfg->compute_dtype != SGL_DTYPE_F32 && cfg->compute_dtype != SGL_DTYPE_BF16 &&
      cfg->compute_dtype != SGL_DTYPE_BF16X3 && cfg->compute_dtype != SGL_DTYPE_F16 &&
      cfg->compute_dtype != SGL_DTYPE_MXFP8)
    return nullptr;
  sgl_ctx* c = new (std::nothrow) sgl_ctx();
  if (!c) return nullptr;
  c->cfg = *cfg;
  c->D = cfg->hidden_size;
  c->I = cfg->intermediate_size;
  c->Ip = round_up(cfg->intermediate_size, 128);
  c->L = cfg->num_layers;
  c->H = cfg->num_heads;
  c->dh = dh;
  c->DP = round_up(dh, 16);
  c->P = cfg->patch_size;
  c->K0 = 3 * c->P * c->P;
  c->Kp = round_up(c->K0, 64);
  c->g0 = cfg->native_grid;
  c->split = cfg->compute_dtype == SGL_DTYPE_BF16X3;
  c->mx = cfg->compute_dtype == SGL_DTYPE_MXFP8;
  c->dt = c->split ? DT_F32 : cfg->compute_dtype == SGL_DTYPE_F16 ? DT_F16 : c->mx ? DT_BF16 : cfg->compute_dtype;
  c->es = dtype_size(c->dt);
  c->Dp = round_up(c->D, 128);
  c->recompute = recompute;
  const size_t es = c->es, D = c->D, Ip = c->Ip, Dp = c->Dp;
  Bump b;
  c->sh_wpatch = b.take(D * c->Kp * es);
  c->sh_layers.resize(c->L);
  for (int l = 0; l < c->L; ++l) {
    ShadowLayer& s = c->sh_layers[l];
    if (c->mx) {   // row-major MX blocks only (no backward, so no transposes); fp32 biases as in the other modes
      s = ShadowLayer{};
      s.wqkv = b.take(3 * D * Dp);
      s.wqkv_s = b.take(3 * D * Dp / 32);
      s.wo = b.take(D * Dp);
      s.wo_s = b.take(D * Dp / 32);
      s.w1 = b.take(Ip * Dp);
      s.w1_s = b.take(Ip * Dp / 32);
      s.w2 = b.take(D * Ip);
      s.w2_s = b.take(D * Ip / 32);
      s.bqkv = b.take(3 * D * 4);
      s.b1 = b.take(Ip * 4);
      continue;
    }
    s.wqkv = b.take(3 * D * D * es);
    s.wqkv_t = b.take(3 * D * D * es);
    s.wo = b.take(D * D * es);
    s.wo_t = b.take(D * D * es);
    s.w1 = b.take(Ip * D * es);
    s.w1_t = b.take(Ip * D * es);
    s.w2 = b.take(Ip * D * es);
    s.w2_t = b.take(Ip * D * es);
    s.bqkv = b.take(3 * D * 4);
    s.b1 = b.take(Ip * 4);
  }
  if (cfg->use_head) {
    c->sh_hwkv = b.take(2 * D * D * es);
    c->sh_hwkv_t = b.take(2 * D * D * es);
    c->sh_hwo = b.take(D * D * es);
    c->sh_hwo_t = b.take(D * D * es);
    c->sh_hw1 = b.take(Ip * D * es);
    c->sh_hw1_t = b.take(Ip * D * es);
    c->sh_hw2 = b.take(Ip * D * es);
    c->sh_hw2_t = b.take(Ip * D * es);
    c->sh_hb1 = b.take(Ip * 4);
  }
  c->sh_total = b.off;
  return c;
}

void sgl_destroy(sgl_ctx* ctx) { delete ctx; }

int sgl_last_hip_error(const sgl_ctx* ctx) { return ctx ? ctx->last_hip : 0; }

int sgl_query_sizes(const sgl_ctx* ctx, int B, int H, int W, int train, size_t* shadow_bytes, size_t* saved_bytes,
                    size_t* ws_bytes) {
  if (!ctx) return SGL_ERR_NULL;
  if (!(train ? train_shape_ok(ctx, B, H, W) : shape_ok(ctx, B, H, W))) return SGL_ERR_BAD_SHAPE;
  if (ctx->mx && train) return SGL_ERR_UNSUPPORTED;   // the MX-fp8 mode has no backward
  Layout lay(ctx, B, H, W, train != 0);
  if (shadow_bytes) *shadow_bytes = ctx->sh_total;
  if (saved_bytes) *saved_bytes = lay.saved_total;
  if (ws_bytes) *ws_bytes = lay.ws_total;
  return SGL_OK;
}

// ---- the placement table: where each master tensor's copies live in the shadow arena -------------------------------
// The ONE statement of it.  sgl_prepare_weights_dirty builds its cast jobs from these records and sgl_adamw_bind_shadows
// hands the same records to the optimizer (optimizer.hip, adamw_ex_kernel), so the two routes that write the arena
// cannot disagree about an offset, a leading dimension or a padding.
struct ShadowMat {
  const float* master;   // fp32 [rows][cols], leading dimension lds
  int rows, cols, lds;
  int row0;              // the copies hold rows [row0, rows)
  size_t dst, dst_t;     // byte offsets of the row-major copy [Rp][Cp] and of the transposed copy [Cp][Rp] (if ld_t != 0)
  int ld, ld_t;          // their leading dimensions, in elements
  int Rp, Cp;            // padded extents: zero outside the (rows - row0) x cols source
};
struct ShadowVec {       // fp32 copy of n elements, zero padded to np
  const float* master;
  int n;
  size_t dst;
  int np;
};
struct ShadowUnit {
  ShadowMat m[6];
  ShadowVec v[4];
  int nm = 0, nv = 0;
};

// unit = block l >= 0, or -1: the globals (patch weight and, with the pooling head, its matrices).  MX mode keeps the
// blocks' matrices as MX operands (quantize_mx, below): a block then has its bias vectors only.
static ShadowUnit shadow_unit(const sgl_ctx* ctx, const sgl_weights* w, int unit) {
  const int D = ctx->D, I = ctx->I, Ip = ctx->Ip;
  const size_t es = ctx->es;
  ShadowUnit u;
  auto square = [&](const float* master, size_t dst, size_t dst_t, int ld_t) {   // [D][D] -> [D][D]
    u.m[u.nm++] = {master, D, D, D, 0, dst, dst_t, D, ld_t, D, D};
  };
  auto mlp = [&](const float* fc1_w, size_t w1, size_t w1_t, const float* fc2_w, size_t w2, size_t w2_t,
                 const float* fc1_b, size_t b1) {   // the intermediate dimension is padded to Ip
    u.m[u.nm++] = {fc1_w, I, D, D, 0, w1, w1_t, D, Ip, Ip, D};
    u.m[u.nm++] = {fc2_w, D, I, I, 0, w2, w2_t, Ip, D, D, Ip};
    u.v[u.nv++] = {fc1_b, I, b1, Ip};
  };
  if (unit >= 0) {
    const sgl_layer_weights& lw = w->layers[unit];
    const ShadowLayer& sl = ctx->sh_layers[unit];
    const float* qkv_w[3] = {lw.q_w, lw.k_w, lw.v_w};
    const float* qkv_b[3] = {lw.q_b, lw.k_b, lw.v_b};
    for (int j = 0; j < 3; ++j) {   // fused: [3D][D] row-major, [D][3D] transposed
      if (!ctx->mx) square(qkv_w[j], sl.wqkv + (size_t)j * D * D * es, sl.wqkv_t + (size_t)j * D * es, 3 * D);
      u.v[u.nv++] = {qkv_b[j], D, sl.bqkv + (size_t)j * D * 4, D};
    }
    if (ctx->mx) {
      u.v[u.nv++] = {lw.fc1_b, I, sl.b1, Ip};
      return u;
    }
    square(lw.o_w, sl.wo, sl.wo_t, D);
    mlp(lw.fc1_w, sl.w1, sl.w1_t, lw.fc2_w, sl.w2, sl.w2_t, lw.fc1_b, sl.b1);
    return u;
  }
  u.m[u.nm++] = {w->patch_w, D, ctx->K0, ctx->K0, 0, ctx->sh_wpatch, 0, ctx->Kp, 0, D, ctx->Kp};   // no transposed copy
  if (ctx->cfg.use_head) {
    // the probe's query never changes with the input: only the k / v rows [D, 3D) of in_proj_w have copies
    u.m[u.nm++] = {w->in_proj_w, 3 * D, D, D, D, ctx->sh_hwkv, ctx->sh_hwkv_t, D, 2 * D, 2 * D, D};
    square(w->out_proj_w, ctx->sh_hwo, ctx->sh_hwo_t, D);
    mlp(w->head_fc1_w, ctx->sh_hw1, ctx->sh_hw1_t, w->head_fc2_w, ctx->sh_hw2, ctx->sh_hw2_t, w->head_fc1_b, ctx->sh_hb1);
  }
  return u;
}

// one launch per unit (elementwise.hip, cast_job_kernel): every matrix read once, written row-major and transposed
static hipError_t cast_unit(const ShadowUnit& u, void* shadow, int dt, hipStream_t s) {
  CastJob job;
  for (int k = 0; k < u.nm; ++k) {
    const ShadowMat& m = u.m[k];
    cast_job_add(job, m.master + (size_t)m.row0 * m.lds, m.rows - m.row0, m.cols, m.lds, at(shadow, m.dst), m.Rp, m.Cp,
                 m.ld, m.ld_t ? at(shadow, m.dst_t) : nullptr, m.ld_t);
  }
  for (int k = 0; k < u.nv; ++k)
    cast_job_add_vec(job, u.v[k].master, u.v[k].n, reinterpret_cast<float*>(at(shadow, u.v[k].dst)), u.v[k].np);
  return cast_job_run(job, dt, s);
}

// layer_dirty: L flags (NULL = every block); globals_dirty: patch embedding + pooling-head matrices.  Frozen-prefix
// fine-tuning (Siglip2sidafrozen.py:757-768) changes 6 of 27 blocks per step: re-casting all of them every step was
// 2.5 % of that config's step.
int sgl_prepare_weights_dirty(sgl_ctx* ctx, const sgl_weights* w, void* shadow, size_t shadow_bytes,
                              const unsigned char* layer_dirty, int globals_dirty, sgl_stream stream) {
  if (!ctx || !w || !shadow || (ctx->L > 0 && !w->layers)) return SGL_ERR_NULL;
  if (shadow_bytes < ctx->sh_total) return SGL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  for (int l = 0; l < ctx->L; ++l) {
    if (layer_dirty && !layer_dirty[l]) continue;
    if (ctx->mx) {   // each weight row quantized along its input dim, exactly as the activations are
      const int D = ctx->D, I = ctx->I, Ip = ctx->Ip;
      const sgl_layer_weights& lw = w->layers[l];
      const ShadowLayer& sl = ctx->sh_layers[l];
      const float* qkv_w[3] = {lw.q_w, lw.k_w, lw.v_w};
      const size_t Dp = ctx->Dp;
      for (int j = 0; j < 3; ++j)
        CK(quantize_mx(qkv_w[j], DT_F32, D, D, D, (int)Dp, at(shadow, sl.wqkv + (size_t)j * D * Dp),
                       at(shadow, sl.wqkv_s + (size_t)j * D * Dp / 32), s));
      CK(quantize_mx(lw.o_w, DT_F32, D, D, D, (int)Dp, at(shadow, sl.wo), at(shadow, sl.wo_s), s));
      CK(quantize_mx(lw.fc1_w, DT_F32, D, I, D, (int)Dp, at(shadow, sl.w1), at(shadow, sl.w1_s), s));
      if (Ip > I) {   // fc1 rows I..Ip: zero bytes and zero scales (their GELU outputs are the zero K-padding of fc2)
        CK(hipMemsetAsync(at(shadow, sl.w1 + (size_t)I * Dp), 0, (size_t)(Ip - I) * Dp, s));
        CK(hipMemsetAsync(at(shadow, sl.w1_s + (size_t)I * Dp / 32), 0, (size_t)(Ip - I) * Dp / 32, s));
      }
      CK(quantize_mx(lw.fc2_w, DT_F32, I, D, I, Ip, at(shadow, sl.w2), at(shadow, sl.w2_s), s));
    }
    CK(cast_unit(shadow_unit(ctx, w, l), shadow, ctx->dt, s));
  }
  if (globals_dirty) CK(cast_unit(shadow_unit(ctx, w, -1), shadow, ctx->dt, s));
  return SGL_OK;
}

int sgl_prepare_weights(sgl_ctx* ctx, const sgl_weights* w, void* shadow, size_t shadow_bytes, sgl_stream stream) {
  return sgl_prepare_weights_dirty(ctx, w, shadow, shadow_bytes, nullptr, 1, stream);
}

// Lets the optimizer write the copies in its own pass: every table entry whose .p is a master of the placement table
// gets that record's destinations.
int sgl_adamw_bind_shadows(const sgl_ctx* ctx, const sgl_weights* w, void* shadow, const sgl_adamw_tensor* table,
                           sgl_adamw_aux* aux, int ntensors) {
  if (!ctx || !w || !shadow || !table || !aux) return SGL_ERR_NULL;
  if (ctx->mx) return 0;   // MX shadows are re-quantized by sgl_prepare_weights_dirty (the mode does not train)
  int bound = 0;
  for (int unit = -1; unit < (w->layers ? ctx->L : 0); ++unit) {
    const ShadowUnit u = shadow_unit(ctx, w, unit);
    for (int i = 0; i < ntensors; ++i) {
      if (!table[i].p) continue;
      for (int k = 0; k < u.nm; ++k) {
        const ShadowMat& m = u.m[k];
        if (table[i].p != m.master) continue;
        aux[i].dst = at(shadow, m.dst);
        aux[i].dst_t = m.ld_t ? at(shadow, m.dst_t) : nullptr;
        aux[i].dst_f32 = nullptr;
        aux[i].ld = m.ld; aux[i].ld_t = m.ld_t; aux[i].rows = m.rows; aux[i].cols = m.cols; aux[i].row0 = m.row0;
        aux[i].dtype = ctx->dt;
        ++bound;
      }
      for (int k = 0; k < u.nv; ++k) {
        if (table[i].p != u.v[k].master) continue;
        aux[i].dst = aux[i].dst_t = nullptr;
        aux[i].dst_f32 = reinterpret_cast<float*>(at(shadow, u.v[k].dst));
        ++bound;
      }
    }
  }
  return bound;
}

// -------------------------------------------------------------------------------------------------------
int sgl_forward_ex(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const float* pixels, int channels_last, int B,
                   int H, int W, int interpolate_pos, float* hidden_states, int hs_slots, float* last_hidden,
                   float* pooled, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, int first_trainable_block,
                   sgl_stream stream);
int sgl_forward_slots(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const float* pixels, int channels_last,
                      int B, int H, int W, int interpolate_pos, float* const* hs_slots, float* last_hidden,
                      float* pooled, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                      int first_trainable_block, sgl_stream stream);

int sgl_forward(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const float* pixels, int channels_last, int B,
                int H, int W, int interpolate_pos, float* hidden_states, int hs_slots, float* last_hidden,
                float* pooled, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream) {
  return sgl_forward_ex(ctx, w, shadow, pixels, channels_last, B, H, W, interpolate_pos, hidden_states, hs_slots,
                        last_hidden, pooled, saved, saved_bytes, ws, ws_bytes, 0, stream);
}

// first_trainable_block: blocks below it will never be differentiated (frozen prefix), so the forward does not write
// their GELU pre-activations (406 MB per block at B = 64); inference (saved == NULL) never writes them.
int sgl_forward_ex(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const float* pixels, int channels_last, int B,
                   int H, int W, int interpolate_pos, float* hidden_states, int hs_slots, float* last_hidden,
                   float* pooled, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, int first_trainable_block,
                   sgl_stream stream) {
  if (!ctx || !hidden_states) return SGL_ERR_NULL;
  if (!shape_ok(ctx, B, H, W)) return SGL_ERR_BAD_SHAPE;
  if (hs_slots < 2 || (saved && hs_slots < ctx->L + 1)) return SGL_ERR_BAD_SHAPE;
  const size_t hs_stride = (size_t)B * (H / ctx->P) * (W / ctx->P) * ctx->D;
  float* slots[kMaxLayers + 1];
  for (int l = 0; l <= ctx->L; ++l) slots[l] = hidden_states + (size_t)(l % hs_slots) * hs_stride;
  return sgl_forward_slots(ctx, w, shadow, pixels, channels_last, B, H, W, interpolate_pos, slots, last_hidden,
                           pooled, saved, saved_bytes, ws, ws_bytes, first_trainable_block, stream);
}

int sgl_forward_slots(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const float* pixels, int channels_last,
                      int B, int H, int W, int interpolate_pos, float* const* hs_slots, float* last_hidden,
                      float* pooled, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                      int first_trainable_block, sgl_stream stream) {
  if (!ctx || !w || !shadow || !pixels || !hs_slots || !last_hidden || (ctx->L > 0 && !w->layers))
    return SGL_ERR_NULL;
  // the slot table's own checks report after a bad shape and around the mode check, both of which begin_call repeats
  if (!shape_ok(ctx, B, H, W)) return SGL_ERR_BAD_SHAPE;
  for (int l = 0; l <= ctx->L; ++l)
    if (!hs_slots[l]) return SGL_ERR_NULL;
  const bool train = saved != nullptr;
  if (train && ctx->mx) return SGL_ERR_UNSUPPORTED;   // the MX-fp8 mode has no backward
  if (train)   // backward reads every hidden state: the slots must be distinct buffers
    for (int l = 0; l < ctx->L; ++l)
      for (int k = l + 1; k <= ctx->L; ++k)
        if (hs_slots[l] == hs_slots[k]) return SGL_ERR_BAD_SHAPE;
  Call c;
  RET(begin_call(c, FORWARD, ctx, shadow, B, H, W, saved, saved_bytes, ws, ws_bytes, stream));
  const Layout& lay = c.lay;
  if (!(lay.gh == ctx->g0 && lay.gw == ctx->g0) && !interpolate_pos) return SGL_ERR_BAD_SHAPE;

  RET(embed_forward(c, w, pixels, channels_last, H, W, hs_slots[0]));
  for (int l = 0; l < ctx->L; ++l) {
    const sgl_layer_weights& lw = w->layers[l];
    const ShadowLayer& sl = ctx->sh_layers[l];
    char* lb = c.block(l);
    if (ctx->mx) {
      RET(mx_block(c, lw, sl, lb, hs_slots[l], hs_slots[l + 1]));
      continue;
    }
    // u is kept for the blocks the backward will differentiate, unless it recomputes them
    RET(block_to_fc1(c, lw, sl, lb, hs_slots[l], train && !lay.rc && l >= first_trainable_block));
    CK(c.gemm_nt(lb + lay.r_a, ctx->Ip, c.sh(sl.w2), ctx->Ip, lay.M, ctx->D, ctx->Ip, EPI_RES_F32, DT_F32,
                 epi_res_f32(hs_slots[l + 1], lw.fc2_b, reinterpret_cast<const float*>(lb + lay.r_xmid), ctx->D)));
  }
  float* pst = c.actf(lay.a_pstats);
  CK(layernorm_fwd(hs_slots[ctx->L], w->post_ln_w, w->post_ln_b, last_hidden, DT_F32, ctx->D, pst, pst + lay.M, lay.M,
                   ctx->D, ctx->cfg.layer_norm_eps, c.s));
  if (ctx->cfg.use_head && pooled) RET(head_forward(c, w, last_hidden, pooled));
  return SGL_OK;
}

// -------------------------------------------------------------------------------------------------------
// ragged batches (inference): S images of different grids packed into one (B = 1, N = T) pass
// -------------------------------------------------------------------------------------------------------
namespace {

// The shape rules of a ragged batch, in the order they are reported: S, every grid side, the token limit, the pooling
// head's per-image limit, and what the context's attention route refuses for the longest image.
int ragged_shape(const sgl_ctx* ctx, const int* grids, int S, int& T, int& max_n) {
  if (S < 1) return SGL_ERR_BAD_SHAPE;
  for (int s = 0; s < S; ++s)
    if (grids[2 * s] < 1 || grids[2 * s + 1] < 1) return SGL_ERR_BAD_SHAPE;
  const long cap = max_tokens(ctx, false);
  long total = 0, longest = 0;
  for (int s = 0; s < S; ++s) {
    const long n = (long)grids[2 * s] * grids[2 * s + 1];
    total += n;
    if (n > longest) longest = n;
    if (total > cap) return SGL_ERR_BAD_SHAPE;
  }
  if (ctx->cfg.use_head && longest > pool_attn_max_tokens(ctx->DP, 0)) return SGL_ERR_BAD_SHAPE;
  T = (int)total;
  max_n = (int)longest;
  if (!attn_varlen_shape_ok(ctx->split ? DT_F32_MFMA : ctx->dt, S, T, max_n, ctx->H, ctx->dh, ctx->DP))
    return SGL_ERR_BAD_SHAPE;
  return SGL_OK;
}

// The packed position table [T][D]: per segment the stored table (native grid), a copy of an earlier segment of the same
// grid, or the table resized to the segment's grid: what embed_forward adds for that image alone.
int ragged_positions(const Call& c, const sgl_weights* w, const int* grids, const std::vector<int>& row0, float* pos) {
  sgl_ctx* ctx = c.ctx;
  const size_t D = (size_t)ctx->D;
  for (int s = 0; s < c.S; ++s) {
    const int gh = grids[2 * s], gw = grids[2 * s + 1];
    float* dst = pos + (size_t)row0[s] * D;
    const size_t bytes = (size_t)gh * gw * D * 4;
    const float* src = (gh == ctx->g0 && gw == ctx->g0) ? w->pos : nullptr;
    for (int e = 0; e < s && !src; ++e)
      if (grids[2 * e] == gh && grids[2 * e + 1] == gw) src = pos + (size_t)row0[e] * D;
    if (src)
      CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c.s));
    else
      CK(pos_resize(w->pos, ctx->g0, dst, gh, gw, ctx->D, c.s));
  }
  return SGL_OK;
}

}  // namespace

int sgl_query_sizes_ragged(const sgl_ctx* ctx, const int* grids, int S, size_t* ws_bytes) {
  if (!ctx || !grids) return SGL_ERR_NULL;
  int T, max_n;
  RET(ragged_shape(ctx, grids, S, T, max_n));
  if (ws_bytes) *ws_bytes = Layout::ragged(ctx, T, S).ws_total;
  return SGL_OK;
}

int sgl_forward_ragged(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const void* patches, const int* grids, int S,
                       float* const* hs_slots, float* last_hidden, float* pooled, void* ws, size_t ws_bytes,
                       sgl_stream stream) {
  if (!ctx || !w || !shadow || !patches || !grids || !hs_slots || !last_hidden || !ws || (ctx->L > 0 && !w->layers))
    return SGL_ERR_NULL;
  int T, max_n;
  RET(ragged_shape(ctx, grids, S, T, max_n));
  for (int l = 0; l <= ctx->L; ++l)
    if (!hs_slots[l]) return SGL_ERR_NULL;
  Call c;
  c.lay = Layout::ragged(ctx, T, S);
  const Layout& lay = c.lay;
  if (ws_bytes < lay.ws_total) return SGL_ERR_WORKSPACE;
  c.ctx = ctx;
  c.s = (hipStream_t)stream;
  c.shadow = shadow;
  c.ws = ws;
  c.act = at(ws, lay.ws_act_off);
  if (ctx->split) {
    c.sp_a = c.act + lay.a_spa;
    c.sp_b = c.act + lay.a_spb;
  }
  c.S = S;
  c.max_n = max_n;
  std::vector<int> lens(S), row0(S);
  for (int s = 0, run = 0; s < S; ++s) {
    lens[s] = grids[2 * s] * grids[2 * s + 1];
    row0[s] = run;
    run += lens[s];
  }
  int* cu = reinterpret_cast<int*>(c.act + lay.a_cu);
  CK(seg_offsets(lens.data(), S, cu, c.s));
  c.cu = cu;

  float* pos = c.actf(lay.a_pos);
  RET(ragged_positions(c, w, grids, row0, pos));
  // `patches` is the GEMM's operand as it stands (inference keeps no copy); every row has its own position row
  CK(c.gemm_nt(patches, ctx->Kp, c.sh(ctx->sh_wpatch), ctx->Kp, T, ctx->D, ctx->Kp, EPI_POS_F32, DT_F32,
               epi_pos_f32(hs_slots[0], ctx->D, w->patch_b, pos, T)));
  for (int l = 0; l < ctx->L; ++l) {
    const sgl_layer_weights& lw = w->layers[l];
    const ShadowLayer& sl = ctx->sh_layers[l];
    char* lb = c.block(l);
    if (ctx->mx) {
      RET(mx_block(c, lw, sl, lb, hs_slots[l], hs_slots[l + 1]));
      continue;
    }
    RET(block_to_fc1(c, lw, sl, lb, hs_slots[l], false));
    CK(c.gemm_nt(lb + lay.r_a, ctx->Ip, c.sh(sl.w2), ctx->Ip, lay.M, ctx->D, ctx->Ip, EPI_RES_F32, DT_F32,
                 epi_res_f32(hs_slots[l + 1], lw.fc2_b, reinterpret_cast<const float*>(lb + lay.r_xmid), ctx->D)));
  }
  float* pst = c.actf(lay.a_pstats);
  CK(layernorm_fwd(hs_slots[ctx->L], w->post_ln_w, w->post_ln_b, last_hidden, DT_F32, ctx->D, pst, pst + lay.M, lay.M,
                   ctx->D, ctx->cfg.layer_norm_eps, c.s));
  if (ctx->cfg.use_head && pooled) RET(head_forward(c, w, last_hidden, pooled));
  return SGL_OK;
}

// -------------------------------------------------------------------------------------------------------
// backward
// -------------------------------------------------------------------------------------------------------
namespace {

// A request for a gradient-weighted attention map (sgl_backward_*_pa), checked before the step enqueues anything.
// block: a block's (N x N) maps; otherwise the pooling head's probe row.
int check_attn_grad_req(const Call& c, const sgl_attn_grad_req* req, bool block, bool available) {
  if (!req) return SGL_OK;
  sgl_ctx* ctx = c.ctx;
  if (!req->out) return SGL_ERR_NULL;
  if (ctx->recompute || ctx->mx || !available) return SGL_ERR_UNSUPPORTED;
  if (req->mode != SGL_ATTN_PROBS_FULL && req->mode != SGL_ATTN_PROBS_HEAD_MEAN) return SGL_ERR_UNSUPPORTED;
  if (req->kind != SGL_ATTN_GRAD_DP && req->kind != SGL_ATTN_GRAD_PDP && req->kind != SGL_ATTN_GRAD_RELEVANCE)
    return SGL_ERR_UNSUPPORTED;
  // a block's launch has its own grid limit: refused here, not after the step's first GEMM is enqueued
  const size_t rows = block ? (size_t)c.lay.N : 1;
  if (block && !attn_grad_probs_shape_ok(ctx->split ? DT_F32_MFMA : ctx->dt, c.lay.B, ctx->H, c.lay.N, ctx->dh, ctx->DP))
    return SGL_ERR_BAD_SHAPE;
  const size_t heads = req->mode == SGL_ATTN_PROBS_FULL ? (size_t)ctx->H : 1;
  if (req->out_bytes < (size_t)c.lay.B * heads * rows * (size_t)c.lay.N * sizeof(float)) return SGL_ERR_WORKSPACE;
  return SGL_OK;
}

// Pooling head backward from d_pooled: the head's parameter gradients, and dlast [M][D] = the gradient w.r.t. the
// post_layernorm output, d_last_hidden (nullable) included
int head_backward(const Call& c, const sgl_weights* w, const sgl_grads* g, const float* d_pooled,
                  const float* d_last_hidden, float* dlast, const sgl_attn_grad_req* req) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, I = ctx->I, Ip = ctx->Ip, M = lay.M, B = lay.B, dt = ctx->dt;
  const int acc = g->accumulate;
  const char* act = c.act;
  const char* kv = act + lay.a_kvh;
  const float* qp = c.actf(lay.a_qp);
  void* hg = c.wsp(lay.w_hg);
  void* hdu = c.wsp(lay.w_hdu);
  void* hdh = c.wsp(lay.w_hdh);
  float* hdao = c.wsf(lay.w_hdao);
  // pooled = h0 + fc2(gelu(fc1(LN(h0))))
  CK(cast_f32(d_pooled, hg, dt, (size_t)B * D, s));
  CK(c.gemm_nt(hg, D, c.sh(ctx->sh_hw2_t), D, B, Ip, D, EPI_GELU_BWD, dt, epi_gelu_bwd(hdu, act + lay.a_hu, Ip, 0)));
  if (g->head_fc2_w) CK(c.gemm_tn(hg, D, act + lay.a_ha, Ip, B, D, I, g->head_fc2_w, I, acc, false));
  RET(c.bias_grad(hg, D, B, D, D, g->head_fc2_b, acc));
  CK(c.gemm_nt(hdu, Ip, c.sh(ctx->sh_hw1_t), Ip, B, D, Ip, EPI_STORE, dt, epi_store(hdh, D)));
  if (g->head_fc1_w) CK(c.gemm_tn(hdu, Ip, act + lay.a_hl, D, B, I, D, g->head_fc1_w, D, acc, false));
  RET(c.bias_grad(hdu, Ip, B, Ip, I, g->head_fc1_b, acc));
  // LN backward (+ residual d_pooled): dh0, low-precision copy into hg
  RET(c.ln_backward(hdh, dt, c.actf(lay.a_h0), c.actf(lay.a_hstats), B, w->head_ln_w, d_pooled, c.wsf(lay.w_hdh0), hg,
                    g->head_ln_w, g->head_ln_b, acc));
  // h0 = ao · Woᵀ + bo
  CK(c.gemm_nt(hg, D, c.sh(ctx->sh_hwo_t), D, B, D, D, EPI_F32, DT_F32, epi_f32(hdao, D)));
  if (g->out_proj_w) CK(c.gemm_tn(hg, D, act + lay.a_ao, D, B, D, D, g->out_proj_w, D, acc, false));
  RET(c.bias_grad(hg, D, B, D, D, g->out_proj_b, acc));
  if (req)
    CK(pool_attn_grad_probs(kv + c.head_bytes(), dt, c.actf(lay.a_probs), hdao, req->out, B, ctx->H, lay.N, ctx->dh,
                            ctx->DP, req->kind, req->mode, s));
  // attention pool backward
  void* dkv = c.wsp(lay.w_dqkv);  // [M][2D]
  float* dqpart = c.wsf(lay.w_hdqpart);
  float* dqp = c.wsf(lay.w_hdqp);
  CK(pool_attn_bwd(qp, kv, kv + c.head_bytes(), dt, c.actf(lay.a_probs), hdao, dkv, dqpart, B, ctx->H, lay.N, ctx->dh,
                   ctx->DP, s));
  if (g->probe || g->in_proj_w || g->in_proj_b) {
    CK(batch_sum(dqpart, B, (size_t)D, dqp, 0, s));
    if (g->in_proj_w)   // d Wq[i,j] = dqp[i] * probe[j]
      CK(gemm_f32_generic(dqp, 1, 1, w->probe, 1, 1, D, D, 1, EPI_F32, DT_F32, epi_f32_acc(g->in_proj_w, D, acc), s));
    if (g->in_proj_b) CK(batch_sum(dqp, 1, (size_t)D, g->in_proj_b, acc, s));
    if (g->probe)   // dprobe[j] = sum_i dqp[i] Wq[i,j]
      CK(gemm_f32_generic(dqp, D, 1, w->in_proj_w, 1, D, 1, D, D, EPI_F32, DT_F32, epi_f32_acc(g->probe, D, acc), s));
  }
  // k,v projections: dlast (+)= dkv · Wkv ; dWkv = dkvᵀ · last_lp
  if (d_last_hidden) CK(copy_f32(d_last_hidden, dlast, (size_t)M * D, s));
  CK(c.gemm_nt(dkv, 2 * D, c.sh(ctx->sh_hwkv_t), 2 * D, M, D, 2 * D, EPI_F32, DT_F32,
               epi_f32_acc(dlast, D, d_last_hidden ? 1 : 0)));
  if (g->in_proj_w)
    CK(c.gemm_tn(dkv, 2 * D, act + lay.a_lastlp, D, M, 2 * D, D, g->in_proj_w + (size_t)D * D, D, acc, true));
  if (g->in_proj_b) RET(c.bias_grad(dkv, 2 * D, M, 2 * D, 2 * D, g->in_proj_b + D, acc));
  return SGL_OK;
}

// A destination whose gradient is identically zero (no_head_grad, i.e. no d_pooled: the pooling head; no_post_ln_grad,
// i.e. neither d_pooled nor d_last_hidden: post_layernorm) is written as zeros when overwriting, like every other
// destination, and left alone when accumulating.
int zero_dead_grads(const Call& c, const sgl_grads* g, bool no_head_grad, bool no_post_ln_grad) {
  sgl_ctx* ctx = c.ctx;
  hipStream_t s = c.s;
  if (g->accumulate) return SGL_OK;
  auto zero = [&](float* p, size_t n) { return p ? hipMemsetAsync(p, 0, n * 4, s) : hipSuccess; };
  const size_t Dz = (size_t)ctx->D, Iz = (size_t)ctx->I;
  if (ctx->cfg.use_head && no_head_grad) {
    CK(zero(g->probe, Dz));
    CK(zero(g->in_proj_w, 3 * Dz * Dz));
    CK(zero(g->in_proj_b, 3 * Dz));
    CK(zero(g->out_proj_w, Dz * Dz));
    CK(zero(g->out_proj_b, Dz));
    CK(zero(g->head_ln_w, Dz));
    CK(zero(g->head_ln_b, Dz));
    CK(zero(g->head_fc1_w, Iz * Dz));
    CK(zero(g->head_fc1_b, Iz));
    CK(zero(g->head_fc2_w, Dz * Iz));
    CK(zero(g->head_fc2_b, Dz));
  }
  if (no_post_ln_grad) {
    CK(zero(g->post_ln_w, Dz));
    CK(zero(g->post_ln_b, Dz));
  }
  return SGL_OK;
}

// The block's MLP: x_out = xmid + fc2(gelu(fc1(LN2 xmid))).  In: gbuf = lowp(d x_out), dx = d x_out, gsum = colsum(dx).
// Out: dx += LN2'(...) = d xmid, gbuf = lowp(dx), gsum = colsum(dx) when the out_proj / v_proj bias gradients are wanted.
int mlp_backward(const Call& c, const sgl_layer_weights& lw, const sgl_layer_grads& lg, const ShadowLayer& sl,
                 const char* lb, int acc) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, I = ctx->I, Ip = ctx->Ip, M = lay.M, dt = ctx->dt;
  float* dx = c.wsf(lay.w_dx);
  void* gbuf = c.wsp(lay.w_g);
  void* du = c.wsp(lay.w_du);
  void* dhb = c.wsp(lay.w_dh);
  float* gsum = c.wsf(lay.w_gsum);   // column sums of dx, left by the producer of dx
  float* csum = c.wsf(lay.w_csum);
  const bool fuse_cs = mfma16(dt) && lg.fc1_b;  // MFMA epilogue adds colsum(du); strict mode uses colsum()
  // deterministic: one row of partial sums per 128-row tile, folded in order below
  if (fuse_cs) CK(hipMemsetAsync(csum, 0, (size_t)((M + 127) / 128) * Ip * 4, s));
  CK(c.gemm_nt(gbuf, D, c.sh(sl.w2_t), D, M, Ip, D, EPI_GELU_BWD, dt,
               epi_gelu_bwd(du, lb + lay.r_u, Ip, mfma16(dt), fuse_cs ? csum : nullptr)));
  if (lg.fc2_w) CK(c.gemm_tn(gbuf, D, lb + lay.r_a, Ip, M, D, I, lg.fc2_w, I, acc, true));
  if (lg.fc2_b) CK(batch_sum(gsum, 1, (size_t)D, lg.fc2_b, acc, s));
  CK(c.gemm_nt(du, Ip, c.sh(sl.w1_t), Ip, M, D, Ip, EPI_STORE, dt, epi_store(dhb, D)));
  if (lg.fc1_w) CK(c.gemm_tn(du, Ip, lb + lay.r_h2, D, M, I, D, lg.fc1_w, D, acc, true));
  if (fuse_cs)
    CK(reduce_partials(csum, (M + 127) / 128, Ip, lg.fc1_b, I, acc, s));
  else
    RET(c.bias_grad(du, Ip, M, Ip, I, lg.fc1_b, acc));
  // LN2 backward: dx := dx + LN2'(dh2);  gbuf := lowp(dx);  colsum(dx) is the out_proj bias gradient
  // (the column sums stay in gsum as well: the v_proj bias gradient below is a function of them)
  RET(c.ln_backward(dhb, dt, reinterpret_cast<const float*>(lb + lay.r_xmid),
                    reinterpret_cast<const float*>(lb + lay.r_stats2), M, lw.ln2_w, dx, dx, gbuf, lg.ln2_w, lg.ln2_b, acc,
                    (lg.o_b || lg.v_b) ? gsum : nullptr));
  if (lg.o_b) CK(batch_sum(gsum, 1, (size_t)D, lg.o_b, acc, s));
  return SGL_OK;
}

// The block's attention: xmid = x_in + out_proj(attn(qkv(LN1 x_in))).  In: gbuf = lowp(d xmid), gsum = colsum(d xmid).
// Out: dqkv [M][3D] and the gradients of out_proj and the three projections; dx is not touched (the residual).
int attn_backward(const Call& c, const sgl_layer_weights& lw, const sgl_layer_grads& lg, const ShadowLayer& sl,
                  const char* lb, int acc, const sgl_attn_grad_req* req) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, M = lay.M, dt = ctx->dt;
  void* gbuf = c.wsp(lay.w_g);
  void* dattn = c.wsp(lay.w_dh);
  void* dqkv = c.wsp(lay.w_dqkv);
  float* gsum = c.wsf(lay.w_gsum);
  const char* q = lb + lay.r_qkv;
  CK(c.gemm_nt(gbuf, D, c.sh(sl.wo_t), D, M, D, D, EPI_STORE, dt, epi_store(dattn, D)));
  // dattn = dO lives until ln1_backward reuses its buffer: the one point where q, k, v, lse and dO are all at hand
  if (req)
    CK(attn_grad_probs(q, q + c.head_bytes(), q + 2 * c.head_bytes(), dattn, reinterpret_cast<const float*>(lb + lay.r_lse),
                       req->out, ctx->split ? DT_F32_MFMA : dt, lay.B, ctx->H, lay.N, ctx->dh, ctx->DP, req->kind,
                       req->mode, s));
  if (lg.o_w) CK(c.gemm_tn(gbuf, D, lb + lay.r_attn, D, M, D, D, lg.o_w, D, acc, true));
  CK(attn_bwd(q, q + c.head_bytes(), q + 2 * c.head_bytes(), lb + lay.r_attn, dattn,
              reinterpret_cast<const float*>(lb + lay.r_lse), ctx->split ? DT_F32_MFMA : dt, dqkv, c.wsf(lay.w_delta),
              lay.B, ctx->H, lay.N, ctx->dh, ctx->DP, 0, s));
  float* gw[3] = {lg.q_w, lg.k_w, lg.v_w};
  float* gb[3] = {lg.q_b, lg.k_b, lg.v_b};
  // when the caller laid the three gradients out back to back (the Python host does), q/k/v are one GEMM
  const bool w_adj = gw[0] && gw[1] == gw[0] + (size_t)D * D && gw[2] == gw[1] + (size_t)D * D;
  if (w_adj) CK(c.gemm_tn(dqkv, 3 * D, lb + lay.r_h1, D, M, 3 * D, D, gw[0], D, acc, true));
  for (int j = 0; j < 3; ++j) {
    const char* aj = reinterpret_cast<const char*>(dqkv) + (size_t)j * D * ctx->es;
    if (!w_adj && gw[j]) CK(c.gemm_tn(aj, 3 * D, lb + lay.r_h1, D, M, D, D, gw[j], D, acc, true));
  }
  // Bias gradients of the three projections = column sums of dQ, dK, dV over all tokens.  Only dQ's needs a pass:
  //   sum_n dK[n,:] = sum_q Q[q,:] * scale * (sum_n dS[q,n]) and sum_n dS[q,n] = sum_n P (dP - delta) = delta - delta = 0:
  //     the k_proj bias has NO gradient (softmax is invariant to a per-query shift of the scores) — exact zeros here,
  //     rounding noise around zero in the reference.  The reference's noise is NaN when dS is not finite, though, and an
  //     overflowing pass has to show in every gradient: a non-finite dS or q makes every column sum of dQ = dS K
  //     non-finite, so the zeros are written as 0 * (the column sums of dQ): +0 from finite sums, NaN otherwise;
  //   sum_n dV[n,:] = sum_q dO[q,:] * (sum_n P[q,n]) = sum_q dO[q,:] = colsum(dY) * W_o, and colsum(dY) is the out_proj bias
  //     gradient the LayerNorm backward above already produced (gsum): a 1152-vector times W_o instead of a read of dV.
  // (One column-sum pass over a third of dqkv instead of all of it: 116 -> ~40 us per block at B = 128.)
  if (gb[0]) RET(c.bias_grad(dqkv, 3 * D, M, D, D, gb[0], acc));
  if (gb[2]) CK(vecmat_f32(gsum, lw.o_w, D, D, c.wsf(lay.w_cspart), gb[2], acc, s));
  if (gb[1]) {
    // without a q_proj bias gradient the column sums of dQ go to gsum: its last reader in this block was the line above,
    // and the LN1 backward that follows rewrites it before anything reads it again
    const float* qsum = gb[0];
    if (!qsum) {
      RET(c.bias_grad(dqkv, 3 * D, M, D, D, gsum, 0));
      qsum = gsum;
    }
    CK(zero_unless_nonfinite(qsum, gb[1], D, acc, s));
  }
  return SGL_OK;
}

// LN1 backward: dx := dx + LN1'(dqkv · Wqkv) = d x_in;  gbuf := lowp(dx);  gsum := colsum(dx) for the block below
int ln1_backward(const Call& c, const sgl_layer_weights& lw, const sgl_layer_grads& lg, const ShadowLayer& sl,
                 const char* lb, const float* x_in, int acc) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  const int D = ctx->D, M = lay.M, dt = ctx->dt;
  float* dx = c.wsf(lay.w_dx);
  void* dh1 = c.wsp(lay.w_dh);  // d LN1 output
  CK(c.gemm_nt(c.wsp(lay.w_dqkv), 3 * D, c.sh(sl.wqkv_t), 3 * D, M, D, 3 * D, EPI_STORE, dt, epi_store(dh1, D)));
  RET(c.ln_backward(dh1, dt, x_in, reinterpret_cast<const float*>(lb + lay.r_stats1), M, lw.ln1_w, dx, dx,
                    c.wsp(lay.w_g), lg.ln1_w, lg.ln1_b, acc, c.wsf(lay.w_gsum)));
  return SGL_OK;
}

}  // namespace

int sgl_backward_begin(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int B, int H, int W,
                       const float* hidden_states, const float* d_last_hidden, const float* d_pooled,
                       const float* d_tap_last, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                       sgl_stream stream) {
  if (!ctx || !hidden_states) return SGL_ERR_NULL;
  if (!train_shape_ok(ctx, B, H, W)) return SGL_ERR_BAD_SHAPE;
  const size_t stride = (size_t)B * (H / ctx->P) * (W / ctx->P) * ctx->D;
  return sgl_backward_begin_p(ctx, w, shadow, g, B, H, W, hidden_states + (size_t)ctx->L * stride, d_last_hidden, d_pooled,
                              d_tap_last, saved, saved_bytes, ws, ws_bytes, stream);
}

int sgl_backward_begin_p(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int B, int H, int W,
                         const float* hs_last, const float* d_last_hidden, const float* d_pooled,
                         const float* d_tap_last, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                         sgl_stream stream) {
  return sgl_backward_begin_pa(ctx, w, shadow, g, B, H, W, hs_last, d_last_hidden, d_pooled, d_tap_last, saved,
                               saved_bytes, ws, ws_bytes, stream, nullptr);
}

int sgl_backward_begin_pa(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int B, int H, int W,
                          const float* hs_last, const float* d_last_hidden, const float* d_pooled,
                          const float* d_tap_last, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                          sgl_stream stream, const sgl_attn_grad_req* req) {
  if (!ctx || !w || !shadow || !g || !hs_last) return SGL_ERR_NULL;
  Call c;
  RET(begin_call(c, BACKWARD, ctx, shadow, B, H, W, saved, saved_bytes, ws, ws_bytes, stream));
  RET(check_attn_grad_req(c, req, false, ctx->cfg.use_head && d_pooled));
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, M = lay.M;
  float* dx = c.wsf(lay.w_dx);
  void* gbuf = c.wsp(lay.w_g);
  float* gsum = c.wsf(lay.w_gsum);
  const float* dlast = d_last_hidden;  // gradient w.r.t. post_layernorm output
  if (ctx->cfg.use_head && d_pooled) {
    float* dlast_buf = c.wsf(lay.w_dlast);
    RET(head_backward(c, w, g, d_pooled, d_last_hidden, dlast_buf, req));
    dlast = dlast_buf;
  }
  RET(zero_dead_grads(c, g, !d_pooled, !dlast));
  // post_layernorm backward -> dx (fp32) and its low-precision copy (A operand of the last block's GEMMs)
  if (dlast) {
    RET(c.ln_backward(dlast, DT_F32, hs_last, c.actf(lay.a_pstats), M, w->post_ln_w, d_tap_last, dx, gbuf, g->post_ln_w,
                      g->post_ln_b, g->accumulate, gsum));
  } else if (d_tap_last) {
    CK(copy_f32(d_tap_last, dx, (size_t)M * D, s));
    CK(cast_f32(d_tap_last, gbuf, ctx->dt, (size_t)M * D, s));
    CK(colsum(gbuf, ctx->dt, D, M, D, D, c.wsf(lay.w_cspart), gsum, 0, s));
  } else {
    CK(hipMemsetAsync(dx, 0, (size_t)M * D * 4, s));
    CK(hipMemsetAsync(gbuf, 0, (size_t)M * D * ctx->es, s));
    CK(hipMemsetAsync(gsum, 0, (size_t)D * 4, s));
  }
  return SGL_OK;
}

int sgl_backward_layer(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int layer, int B,
                       int H, int W, const float* hidden_states, const float* d_tap, int need_dx, const void* saved,
                       size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream) {
  if (!ctx || !hidden_states) return SGL_ERR_NULL;
  if (layer < 0 || layer >= ctx->L || !train_shape_ok(ctx, B, H, W)) return SGL_ERR_BAD_SHAPE;
  const size_t stride = (size_t)B * (H / ctx->P) * (W / ctx->P) * ctx->D;
  return sgl_backward_layer_p(ctx, w, shadow, g, layer, B, H, W, hidden_states + (size_t)layer * stride, d_tap, need_dx,
                              saved, saved_bytes, ws, ws_bytes, stream);
}

int sgl_backward_layer_p(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int layer, int B,
                         int H, int W, const float* hs_in, const float* d_tap, int need_dx, const void* saved,
                         size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream) {
  return sgl_backward_layer_pa(ctx, w, shadow, g, layer, B, H, W, hs_in, d_tap, need_dx, saved, saved_bytes, ws, ws_bytes,
                               stream, nullptr);
}

int sgl_backward_layer_pa(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int layer, int B,
                          int H, int W, const float* hs_in, const float* d_tap, int need_dx, const void* saved,
                          size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream,
                          const sgl_attn_grad_req* req) {
  if (!ctx || !w || !shadow || !g || !hs_in || !g->layers || !w->layers) return SGL_ERR_NULL;
  if (layer < 0 || layer >= ctx->L) return SGL_ERR_BAD_SHAPE;
  Call c;
  RET(begin_call(c, BACKWARD, ctx, shadow, B, H, W, saved, saved_bytes, ws, ws_bytes, stream));
  RET(check_attn_grad_req(c, req, true, true));
  const int acc = g->accumulate;
  const sgl_layer_weights& lw = w->layers[layer];
  const sgl_layer_grads& lg = g->layers[layer];
  const ShadowLayer& sl = ctx->sh_layers[layer];
  // recompute context: rebuild the block's activations from its input into the shared region first (everything but fc2:
  // hidden_states[layer + 1] is saved); the region is disjoint from the gradient this call carries in ws
  char* lb = c.block(layer);
  if (c.lay.rc) RET(block_to_fc1(c, lw, sl, lb, hs_in, true));
  RET(mlp_backward(c, lw, lg, sl, lb, acc));
  RET(attn_backward(c, lw, lg, sl, lb, acc, req));
  float* dx = c.wsf(c.lay.w_dx);
  if (d_tap) CK(add_f32(dx, d_tap, dx, (size_t)c.lay.M * ctx->D, c.s));
  if (need_dx || lg.ln1_w || lg.ln1_b) RET(ln1_backward(c, lw, lg, sl, lb, hs_in, acc));
  return SGL_OK;
}

namespace {

// Patch-embedding parameter gradients from d hidden_states[0] (dx fp32 and its low-precision copy gbuf in ws)
int embed_param_backward(const Call& c, const sgl_grads* g) {
  sgl_ctx* ctx = c.ctx;
  const Layout& lay = c.lay;
  hipStream_t s = c.s;
  const int D = ctx->D, M = lay.M, N = lay.N;
  const int acc = g->accumulate;
  float* dx = c.wsf(lay.w_dx);
  void* gbuf = c.wsp(lay.w_g);  // low-precision copy of dx (written by the last LN1 backward / begin)
  if (g->patch_w)
    CK(c.gemm_tn(gbuf, D, c.act + lay.a_im2col, ctx->Kp, M, D, ctx->K0, g->patch_w, ctx->K0, acc, true));
  if (g->patch_b) CK(batch_sum(c.wsf(lay.w_gsum), 1, (size_t)D, g->patch_b, acc, s));
  if (g->pos) {
    if (lay.gh == ctx->g0 && lay.gw == ctx->g0) {
      CK(batch_sum(dx, lay.B, (size_t)N * D, g->pos, acc, s));
    } else {
      float* dpos = c.wsf(lay.w_dlast);  // [N][D] scratch
      CK(batch_sum(dx, lay.B, (size_t)N * D, dpos, 0, s));
      if (!acc) CK(hipMemsetAsync(g->pos, 0, (size_t)ctx->g0 * ctx->g0 * D * 4, s));
      CK(pos_resize_bwd(dpos, lay.gh, lay.gw, g->pos, ctx->g0, D, s));
    }
  }
  return SGL_OK;
}

// The caller's scratch of sgl_backward_embed_px: d_cols [M][Kp] fp32 (the patch GEMM's dX), then W_patch^T [Kp][D] in the
// compute dtype (rows K0 .. Kp zero).  The bf16x3 split of that one product (A [M][D], B [Kp][D]) is never wider than the
// operands the call's own split scratch is sized for (Layout: sp_act / sp_wgt), so it needs no room here.
struct PxLayout {
  size_t dcols = 0, wpt = 0, total = 0;
  PxLayout(const sgl_ctx* c, int M) {
    Bump b;
    dcols = b.take((size_t)M * c->Kp * 4);
    wpt = b.take((size_t)c->Kp * c->D * c->es);
    total = b.off;
  }
};

}  // namespace

int sgl_backward_embed(sgl_ctx* ctx, const sgl_weights* w, const sgl_grads* g, int B, int H, int W, int interpolate_pos,
                       const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream) {
  if (!ctx || !w || !g) return SGL_ERR_NULL;
  Call c;
  RET(begin_call(c, BACKWARD, ctx, nullptr, B, H, W, saved, saved_bytes, ws, ws_bytes, stream));
  (void)interpolate_pos;
  return embed_param_backward(c, g);
}

int sgl_query_input_grad_bytes(const sgl_ctx* ctx, int B, int H, int W, size_t* scratch_bytes) {
  if (!ctx || !scratch_bytes) return SGL_ERR_NULL;
  if (!train_shape_ok(ctx, B, H, W)) return SGL_ERR_BAD_SHAPE;
  if (ctx->mx) return SGL_ERR_UNSUPPORTED;   // the MX-fp8 mode has no backward
  *scratch_bytes = PxLayout(ctx, B * (H / ctx->P) * (W / ctx->P)).total;
  return SGL_OK;
}

// sgl_backward_embed, then d_pixels = col2im(lowp(d hidden_states[0]) . W_patch): the patch GEMM's dX as an NT GEMM against
// the transposed patch weight, which is cast per call into the caller's scratch (no shadow of it exists)
int sgl_backward_embed_px(sgl_ctx* ctx, const sgl_weights* w, const sgl_grads* g, int B, int H, int W,
                          int interpolate_pos, float* d_pixels, int channels_last, void* px_scratch,
                          size_t px_scratch_bytes, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                          sgl_stream stream) {
  if (!ctx || !w || !g || !w->patch_w) return SGL_ERR_NULL;
  if (!d_pixels || !px_scratch) return SGL_ERR_NULL;
  if (channels_last != 0 && channels_last != 1) return SGL_ERR_UNSUPPORTED;   // a ready patch operand has no pixels
  Call c;
  RET(begin_call(c, BACKWARD, ctx, nullptr, B, H, W, saved, saved_bytes, ws, ws_bytes, stream));
  const Layout& lay = c.lay;
  const PxLayout px(ctx, lay.M);
  if (px_scratch_bytes < px.total) return SGL_ERR_WORKSPACE;
  (void)interpolate_pos;
  RET(embed_param_backward(c, g));
  const int D = ctx->D, Kp = ctx->Kp;
  float* dcols = reinterpret_cast<float*>(at(px_scratch, px.dcols));
  void* wpt = at(px_scratch, px.wpt);
  CastJob job;   // transposed copy only: wpt[k][d] = cast(patch_w[d][k]), zero for k >= K0
  cast_job_add(job, w->patch_w, D, ctx->K0, ctx->K0, nullptr, D, Kp, Kp, wpt, D);
  CK(cast_job_run(job, ctx->dt, c.s));
  CK(c.gemm_nt(c.wsp(lay.w_g), D, wpt, D, lay.M, Kp, D, EPI_F32, DT_F32, epi_f32(dcols, Kp)));
  CK(col2im(dcols, lay.B, H, W, ctx->P, Kp, d_pixels, channels_last, c.s));
  return SGL_OK;
}

int sgl_backward(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int B, int H, int W,
                 int interpolate_pos, const float* hidden_states, const float* const* d_taps,
                 const float* d_last_hidden, const float* d_pooled, int first_trainable_block, int train_embeddings,
                 const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream) {
  if (!ctx) return SGL_ERR_NULL;
  const int L = ctx->L;
  int stop = train_embeddings ? 0 : first_trainable_block;
  if (stop < 0) stop = 0;
  // what only the per-block step checks is checked here, before sgl_backward_begin enqueues anything
  if (stop < L && w && g && (!w->layers || !g->layers)) return SGL_ERR_NULL;
  RET(sgl_backward_begin(ctx, w, shadow, g, B, H, W, hidden_states, d_last_hidden, d_pooled,
                         d_taps ? d_taps[L] : nullptr, saved, saved_bytes, ws, ws_bytes, stream));
  for (int l = L - 1; l >= stop; --l) {
    const int need_dx = (l > stop) || train_embeddings;
    RET(sgl_backward_layer(ctx, w, shadow, g, l, B, H, W, hidden_states, d_taps ? d_taps[l] : nullptr, need_dx, saved,
                           saved_bytes, ws, ws_bytes, stream));
  }
  if (train_embeddings)
    RET(sgl_backward_embed(ctx, w, g, B, H, W, interpolate_pos, saved, saved_bytes, ws, ws_bytes, stream));
  return SGL_OK;
}

// -------------------------------------------------------------------------------------------------------
// single-kernel entry points
// -------------------------------------------------------------------------------------------------------
#define CKV(expr)                                   \
  do {                                              \
    hipError_t e_ = (expr);                         \
    if (e_ == hipErrorInvalidValue) return SGL_ERR_UNSUPPORTED; \
    if (e_ != hipSuccess) return SGL_ERR_HIP;       \
  } while (0)

int sgl_op_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                         float* rstd, int M, int D, float eps, sgl_stream stream) {
  CKV(layernorm_fwd(x, gamma, beta, y, y_dtype, D, mean, rstd, M, D, eps, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_quantize_mxfp8(const void* x, int x_dtype, int ldx, int M, int K, int Kp, void* q, void* scales,
                          sgl_stream stream) {
  if (!x || !q || !scales) return SGL_ERR_NULL;
  CKV(quantize_mx(x, x_dtype, ldx, M, K, Kp, q, scales, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_layernorm_fwd_mx(const float* x, const float* gamma, const float* beta, void* q, void* scales, int M, int D,
                            int Kp, float eps, sgl_stream stream) {
  if (!x || !gamma || !beta || !q || !scales) return SGL_ERR_NULL;
  CKV(layernorm_fwd_mx(x, gamma, beta, q, scales, M, D, Kp, eps, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_gemm_nt_mx(const void* A, const void* As, const void* B, const void* Bs, int M, int N, int Kp, int epi,
                      void* out, int ldo, void* out_scales, const float* bias, const float* res, int ldr, int tokens,
                      int heads, int head_dim, int head_dim_pad, int batch, sgl_stream stream) {
  if (!A || !As || !B || !Bs || !out || !bias) return SGL_ERR_NULL;
  EpiParams p;
  p.out = out; p.ldo = ldo; p.bias = bias; p.res = res; p.ldr = ldr;
  p.tokens = tokens > 0 ? tokens : 1; p.heads = heads > 0 ? heads : 1; p.head_dim = head_dim > 0 ? head_dim : 8;
  p.head_dim_pad = head_dim_pad > 0 ? head_dim_pad : 8; p.batch = batch > 0 ? batch : 1;
  CKV(gemm_nt_mx(A, As, B, Bs, M, N, Kp, epi, p, out_scales, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* mean, const float* rstd,
                         const float* gamma, const float* dres, float* dx, void* dx_lp, int lp_dtype, float* dgamma,
                         float* dbeta, float* scratch, size_t scratch_bytes, int M, int D, sgl_stream stream) {
  const int nblk = layernorm_bwd_blocks(M);
  if (scratch_bytes < (size_t)nblk * 3 * D * 4) return SGL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  CKV(layernorm_bwd(dy, dy_dtype, D, x, mean, rstd, gamma, dres, dx, dx_lp, lp_dtype, scratch, nblk, M, D, s));
  if (dgamma) CKV(reduce_partials(scratch, nblk, 3 * D, dgamma, D, 0, s));
  if (dbeta) CKV(reduce_partials(scratch + D, nblk, 3 * D, dbeta, D, 0, s));
  return SGL_OK;
}

int sgl_op_gemm_nt(int dtype, const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, void* out,
                   int ldo, void* out2, int ldo2, const float* bias, const float* res, int ldr, const void* aux,
                   int ldaux, const float* pos, int pos_rows, int tokens, int heads, int head_dim, int head_dim_pad,
                   int batch, sgl_stream stream) {
  EpiParams p;
  p.out = out; p.ldo = ldo; p.out2 = out2; p.ldo2 = ldo2; p.bias = bias; p.res = res; p.ldr = ldr;
  p.aux = aux; p.ldaux = ldaux; p.pos = pos; p.pos_rows = pos_rows > 0 ? pos_rows : 1;
  p.tokens = tokens > 0 ? tokens : 1; p.heads = heads > 0 ? heads : 1; p.head_dim = head_dim > 0 ? head_dim : 8;
  p.head_dim_pad = head_dim_pad > 0 ? head_dim_pad : 8; p.batch = batch > 0 ? batch : 1;
  const bool f32_out = (epi == EPI_RES_F32 || epi == EPI_POS_F32 || epi == EPI_F32);
  const int out_dt = f32_out ? DT_F32 : dtype;
  if (dtype == DT_BF16)
    CKV(gemm_nt_bf16(A, lda, B, ldb, M, N, K, epi, out_dt, p, (hipStream_t)stream));
  else if (dtype == DT_F16)
    CKV(gemm_nt_f16(A, lda, B, ldb, M, N, K, epi, out_dt, p, (hipStream_t)stream));
  else
    CKV(gemm_f32_generic((const float*)A, lda, 1, (const float*)B, ldb, 1, M, N, K, epi, out_dt, p,
                         (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_gemm_tn(int dtype, const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                   float* out, int ldo, int accumulate, sgl_stream stream) {
  return sgl_op_gemm_tn_ws(dtype, A, lda, B, ldb, Mred, N1, N2, splits, out, ldo, accumulate, nullptr, 0, stream);
}

int sgl_op_gemm_tn_ws(int dtype, const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                      float* out, int ldo, int accumulate, float* scratch, size_t scratch_bytes, sgl_stream stream) {
  EpiParams p;
  p.out = out; p.ldo = ldo; p.accumulate = accumulate;
  if (dtype == DT_BF16)
    CKV(gemm_tn_bf16(A, lda, B, ldb, Mred, N1, N2, splits, p, (hipStream_t)stream, scratch, scratch_bytes));
  else if (dtype == DT_F16)
    CKV(gemm_tn_f16(A, lda, B, ldb, Mred, N1, N2, splits, p, (hipStream_t)stream, scratch, scratch_bytes));
  else
    CKV(gemm_f32_generic((const float*)A, 1, lda, (const float*)B, 1, ldb, N1, N2, Mred, EPI_F32, DT_F32, p,
                         (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_attn_fwd(int dtype, const void* q, const void* k, const void* v, void* out, float* lse, int B, int H, int N,
                    int head_dim, int head_dim_pad, int ld_qkv, sgl_stream stream) {
  CKV(attn_fwd(q, k, v, dtype, out, lse, B, H, N, head_dim, head_dim_pad, ld_qkv, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* out, const void* dout,
                    const float* lse, void* dqkv, float* delta_scratch, int B, int H, int N, int head_dim,
                    int head_dim_pad, int ld_qkv, sgl_stream stream) {
  CKV(attn_bwd(q, k, v, out, dout, lse, dtype, dqkv, delta_scratch, B, H, N, head_dim, head_dim_pad, ld_qkv, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_attn_probs(int dtype, const void* q, const void* k, const float* lse, float* out, int B, int H, int N,
                      int head_dim, int head_dim_pad, int mode, sgl_stream stream) {
  if (!q || !k || !lse || !out) return SGL_ERR_NULL;
  if (B < 1 || H < 1 || N < 1 || head_dim < 1 || head_dim_pad < 1 || head_dim > head_dim_pad) return SGL_ERR_BAD_SHAPE;
  if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F32_MFMA && dtype != DT_F16) return SGL_ERR_UNSUPPORTED;
  if (mode != SGL_ATTN_PROBS_FULL && mode != SGL_ATTN_PROBS_HEAD_MEAN) return SGL_ERR_UNSUPPORTED;
  if (!attn_probs_shape_ok(dtype, B, H, N, head_dim, head_dim_pad)) return SGL_ERR_BAD_SHAPE;
  CKV(attn_probs(q, k, lse, out, dtype, B, H, N, head_dim, head_dim_pad, mode, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_attn_grad_probs(int dtype, const void* q, const void* k, const void* v, const void* dout, const float* lse,
                           float* out, int B, int H, int N, int head_dim, int head_dim_pad, int kind, int mode,
                           sgl_stream stream) {
  if (!q || !k || !v || !dout || !lse || !out) return SGL_ERR_NULL;
  if (B < 1 || H < 1 || N < 1 || head_dim < 1 || head_dim_pad < 1 || head_dim > head_dim_pad) return SGL_ERR_BAD_SHAPE;
  if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F32_MFMA && dtype != DT_F16) return SGL_ERR_UNSUPPORTED;
  if (mode != SGL_ATTN_PROBS_FULL && mode != SGL_ATTN_PROBS_HEAD_MEAN) return SGL_ERR_UNSUPPORTED;
  if (kind != SGL_ATTN_GRAD_DP && kind != SGL_ATTN_GRAD_PDP && kind != SGL_ATTN_GRAD_RELEVANCE) return SGL_ERR_UNSUPPORTED;
  if (!attn_grad_probs_shape_ok(dtype, B, H, N, head_dim, head_dim_pad)) return SGL_ERR_BAD_SHAPE;
  CKV(attn_grad_probs(q, k, v, dout, lse, out, dtype, B, H, N, head_dim, head_dim_pad, kind, mode, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_attention_probs(sgl_ctx* ctx, int B, int H, int W, const void* saved, size_t saved_bytes, int layer, int mode,
                        float* out, size_t out_bytes, sgl_stream stream) {
  if (!ctx || !saved || !out) return SGL_ERR_NULL;
  if (!train_shape_ok(ctx, B, H, W) || layer < 0 || layer > ctx->L) return SGL_ERR_BAD_SHAPE;
  if (ctx->recompute || ctx->mx || (layer == ctx->L && !ctx->cfg.use_head)) return SGL_ERR_UNSUPPORTED;
  if (mode != SGL_ATTN_PROBS_FULL && mode != SGL_ATTN_PROBS_HEAD_MEAN) return SGL_ERR_UNSUPPORTED;
  const Layout lay(ctx, B, H, W, true);
  const size_t N = (size_t)lay.N, heads = mode == SGL_ATTN_PROBS_FULL ? (size_t)ctx->H : 1;
  const size_t need = (size_t)B * heads * N * (layer == ctx->L ? 1 : N) * sizeof(float);
  if (saved_bytes < lay.saved_total || out_bytes < need) return SGL_ERR_WORKSPACE;
  const char* act = reinterpret_cast<const char*>(saved);
  hipStream_t s = (hipStream_t)stream;
  if (layer == ctx->L) {   // the pooling head kept its probe probabilities [B][heads][N]
    const float* probs = reinterpret_cast<const float*>(act + lay.a_probs);
    if (mode == SGL_ATTN_PROBS_FULL)
      CK(copy_f32(probs, out, (size_t)B * ctx->H * N, s));
    else
      CK(probs_head_mean(probs, out, B, ctx->H, lay.N, s));
    return SGL_OK;
  }
  const char* lb = act + lay.layer_base(layer);
  const char* q = lb + lay.r_qkv;
  CK(attn_probs(q, q + head_bytes(ctx, B, lay.N), reinterpret_cast<const float*>(lb + lay.r_lse), out,
                ctx->split ? DT_F32_MFMA : ctx->dt, B, ctx->H, lay.N, ctx->dh, ctx->DP, mode, s));
  return SGL_OK;
}

int sgl_op_colsum(int dtype, const void* in, int ld, int M, int N, float* out, int accumulate, float* scratch,
                  size_t scratch_bytes, sgl_stream stream) {
  if (scratch_bytes < (size_t)colsum_chunks(M) * N * 4) return SGL_ERR_WORKSPACE;
  CKV(colsum(in, dtype, ld, M, N, N, scratch, out, accumulate, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_im2col(const float* pixels, int channels_last, void* out, int out_dtype, int B, int H, int W, int P, int Kp,
                  sgl_stream stream) {
  CKV(im2col(pixels, channels_last, out, out_dtype, B, H, W, P, Kp, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_col2im(const float* d_cols, int B, int H, int W, int P, int Kp, float* d_pixels, int channels_last,
                  sgl_stream stream) {
  if (!d_cols || !d_pixels) return SGL_ERR_NULL;
  CKV(col2im(d_cols, B, H, W, P, Kp, d_pixels, channels_last, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_pos_resize(const float* table, int native_grid, float* out, int gh, int gw, int D, sgl_stream stream) {
  CKV(pos_resize(table, native_grid, out, gh, gw, D, (hipStream_t)stream));
  return SGL_OK;
}

// -------------------------------------------------------------------------------------------------------
// the kernels only the encoder calls, one thin entry point each (tests and bindings)
// -------------------------------------------------------------------------------------------------------
static bool lo_dtype_ok(int dt) { return dt == DT_F32 || dt == DT_BF16 || dt == DT_F16; }
static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

int sgl_op_pool_attn_fwd(int dtype, const float* q, const void* K, const void* V, void* out, float* probs, int B, int H,
                         int N, int head_dim, int head_dim_pad, sgl_stream stream) {
  if (!q || !K || !V || !out || !probs) return SGL_ERR_NULL;
  if (B <= 0 || H <= 0 || N <= 0 || head_dim <= 0 || head_dim % 8 || head_dim_pad % 8 || head_dim > head_dim_pad)
    return SGL_ERR_BAD_SHAPE;
  if (!lo_dtype_ok(dtype) || !aligned16(K) || !aligned16(V)) return SGL_ERR_UNSUPPORTED;
  CKV(pool_attn_fwd(q, K, V, dtype, out, probs, B, H, N, head_dim, head_dim_pad, (hipStream_t)stream));
  return SGL_OK;
}

// ---- ragged batches: the two varlen kernels and the table writer -----------------------------------------------------
int sgl_op_attn_fwd_varlen(int dtype, const void* q, const void* k, const void* v, void* out, float* lse, const int* cu,
                           int S, int T, int max_n, int H, int head_dim, int head_dim_pad, sgl_stream stream) {
  if (!q || !k || !v || !out || !lse || !cu) return SGL_ERR_NULL;
  if (S < 1 || T < 1 || max_n < 1 || H < 1 || head_dim < 1 || head_dim_pad < 1 || head_dim > head_dim_pad)
    return SGL_ERR_BAD_SHAPE;
  if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F32_MFMA && dtype != DT_F16) return SGL_ERR_UNSUPPORTED;
  if (!attn_varlen_shape_ok(dtype, S, T, max_n, H, head_dim, head_dim_pad)) return SGL_ERR_BAD_SHAPE;
  CKV(attn_fwd_varlen(q, k, v, dtype, out, lse, cu, S, T, max_n, H, head_dim, head_dim_pad, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_pool_attn_fwd_varlen(int dtype, const float* q, const void* K, const void* V, void* out, float* probs,
                                const int* cu, int S, int T, int max_n, int H, int head_dim, int head_dim_pad,
                                sgl_stream stream) {
  if (!q || !K || !V || !out || !probs || !cu) return SGL_ERR_NULL;
  if (S <= 0 || T <= 0 || max_n <= 0 || H <= 0 || head_dim <= 0 || head_dim % 8 || head_dim_pad % 8 ||
      head_dim > head_dim_pad)
    return SGL_ERR_BAD_SHAPE;
  if (!lo_dtype_ok(dtype) || !aligned16(K) || !aligned16(V)) return SGL_ERR_UNSUPPORTED;
  CKV(pool_attn_fwd_varlen(q, K, V, dtype, out, probs, cu, S, T, max_n, H, head_dim, head_dim_pad, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_seg_offsets(const int* lens, int S, int* cu, sgl_stream stream) {
  if (!lens || !cu) return SGL_ERR_NULL;
  if (S < 1) return SGL_ERR_BAD_SHAPE;
  long long total = 0;
  for (int i = 0; i < S; ++i) {
    if (lens[i] < 0) return SGL_ERR_BAD_SHAPE;
    total += lens[i];
  }
  if (total > 0x7fffffffLL) return SGL_ERR_BAD_SHAPE;
  CKV(seg_offsets(lens, S, cu, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_pool_attn_bwd(int dtype, const float* q, const void* K, const void* V, const float* probs, const float* dout,
                         void* dkv, float* dq_partial, int B, int H, int N, int head_dim, int head_dim_pad,
                         sgl_stream stream) {
  if (!q || !K || !V || !probs || !dout || !dkv || !dq_partial) return SGL_ERR_NULL;
  if (B <= 0 || H <= 0 || N <= 0 || head_dim <= 0 || head_dim % 8 || head_dim_pad % 8 || head_dim > head_dim_pad)
    return SGL_ERR_BAD_SHAPE;
  if (!lo_dtype_ok(dtype) || !aligned16(K) || !aligned16(V) || !aligned16(dkv)) return SGL_ERR_UNSUPPORTED;
  CKV(pool_attn_bwd(q, K, V, dtype, probs, dout, dkv, dq_partial, B, H, N, head_dim, head_dim_pad, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_pool_attn_grad_probs(int dtype, const void* V, const float* probs, const float* dout, float* out, int B, int H,
                                int N, int head_dim, int head_dim_pad, int kind, int mode, sgl_stream stream) {
  if (!V || !probs || !dout || !out) return SGL_ERR_NULL;
  if (B <= 0 || H <= 0 || N <= 0 || head_dim <= 0 || head_dim % 8 || head_dim_pad % 8 || head_dim > head_dim_pad)
    return SGL_ERR_BAD_SHAPE;
  if (!lo_dtype_ok(dtype) || !aligned16(V)) return SGL_ERR_UNSUPPORTED;
  if (mode != SGL_ATTN_PROBS_FULL && mode != SGL_ATTN_PROBS_HEAD_MEAN) return SGL_ERR_UNSUPPORTED;
  if (kind != SGL_ATTN_GRAD_DP && kind != SGL_ATTN_GRAD_PDP && kind != SGL_ATTN_GRAD_RELEVANCE) return SGL_ERR_UNSUPPORTED;
  CKV(pool_attn_grad_probs(V, dtype, probs, dout, out, B, H, N, head_dim, head_dim_pad, kind, mode, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_pos_resize_bwd(const float* dout, int gh, int gw, float* dtable, int native_grid, int D, sgl_stream stream) {
  if (!dout || !dtable) return SGL_ERR_NULL;
  if (gh <= 0 || gw <= 0 || native_grid <= 0 || D <= 0) return SGL_ERR_BAD_SHAPE;
  CKV(pos_resize_bwd(dout, gh, gw, dtable, native_grid, D, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_cast_pad(const float* src, int R, int C, int lds, void* dst, int dst_dtype, int Rp, int Cp, int ldd,
                    sgl_stream stream) {
  if (!src || !dst) return SGL_ERR_NULL;
  if (R < 0 || C < 0 || Rp < R || Cp < C || lds < C || ldd < Cp) return SGL_ERR_BAD_SHAPE;
  if (!lo_dtype_ok(dst_dtype)) return SGL_ERR_UNSUPPORTED;
  CKV(cast_pad(src, R, C, lds, dst, dst_dtype, Rp, Cp, ldd, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_cast_job(const sgl_cast_mat* mats, int nmat, const sgl_cast_vec* vecs, int nvec, int dst_dtype,
                    sgl_stream stream) {
  if ((nmat > 0 && !mats) || (nvec > 0 && !vecs)) return SGL_ERR_NULL;
  if (nmat < 0 || nmat > 6 || nvec < 0 || nvec > 4) return SGL_ERR_BAD_SHAPE;
  for (int k = 0; k < nmat; ++k)
    if (!mats[k].src || (!mats[k].dst && !mats[k].dst_t)) return SGL_ERR_NULL;
  for (int k = 0; k < nvec; ++k)
    if (!vecs[k].src || !vecs[k].dst) return SGL_ERR_NULL;
  for (int k = 0; k < nmat; ++k) {
    const sgl_cast_mat& m = mats[k];
    if (m.R <= 0 || m.C <= 0 || m.Rp < m.R || m.Cp < m.C || m.lds < m.C || (m.dst && m.ldd < m.Cp) ||
        (m.dst_t && m.ldt < m.Rp))
      return SGL_ERR_BAD_SHAPE;
  }
  for (int k = 0; k < nvec; ++k)
    if (vecs[k].n < 0 || vecs[k].np < vecs[k].n) return SGL_ERR_BAD_SHAPE;
  if (!lo_dtype_ok(dst_dtype)) return SGL_ERR_UNSUPPORTED;
  CastJob job;
  for (int k = 0; k < nmat; ++k) {
    const sgl_cast_mat& m = mats[k];
    cast_job_add(job, m.src, m.R, m.C, m.lds, m.dst, m.Rp, m.Cp, m.ldd, m.dst_t, m.ldt);
  }
  for (int k = 0; k < nvec; ++k) cast_job_add_vec(job, vecs[k].src, vecs[k].n, vecs[k].dst, vecs[k].np);
  CKV(cast_job_run(job, dst_dtype, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_split3(const float* src, int R, int C, int ld, void* dst, int Cs, int b_side, int stacked, sgl_stream stream) {
  if (!src || !dst) return SGL_ERR_NULL;
  if (R <= 0 || C <= 0 || ld < C || Cs != round_up(C, 8)) return SGL_ERR_BAD_SHAPE;
  if (!aligned16(dst)) return SGL_ERR_UNSUPPORTED;   // 16-byte stores of eight bf16
  if (stacked)
    CKV(split3_stack(src, R, C, ld, dst, Cs, b_side ? 1 : 0, (hipStream_t)stream));
  else
    CKV(split3_rows(src, R, C, ld, dst, Cs, b_side ? 1 : 0, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_batch_sum(const float* in, int B, size_t n, float* out, int accumulate, sgl_stream stream) {
  if (!in || !out) return SGL_ERR_NULL;
  if (B <= 0 || n >= ((size_t)1 << 31) * 256) return SGL_ERR_BAD_SHAPE;   // one thread per element, grid.x < 2^31
  CKV(batch_sum(in, B, n, out, accumulate, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_vecmat(const float* v, const float* W, int rows, int cols, float* scratch, size_t scratch_bytes, float* out,
                  int accumulate, sgl_stream stream) {
  if (!v || !W || !scratch || !out) return SGL_ERR_NULL;
  if (rows <= 0 || cols <= 0) return SGL_ERR_BAD_SHAPE;
  if (scratch_bytes < (size_t)16 * cols * 4) return SGL_ERR_WORKSPACE;
  CKV(vecmat_f32(v, W, rows, cols, scratch, out, accumulate, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_reduce_partials(const float* partial, int nblk, int stride, float* out, int n, int accumulate,
                           sgl_stream stream) {
  if (!partial || !out) return SGL_ERR_NULL;
  if (nblk <= 0 || n <= 0 || stride < n) return SGL_ERR_BAD_SHAPE;
  CKV(reduce_partials(partial, nblk, stride, out, n, accumulate, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_reduce_partials3(const float* partial, int nblk, int stride, float* out0, float* out1, float* out2, int n,
                            int accumulate0, int accumulate1, int accumulate2, sgl_stream stream) {
  if (!partial) return SGL_ERR_NULL;
  if (nblk <= 0 || n <= 0 || stride < 3 * (long)n) return SGL_ERR_BAD_SHAPE;
  CKV(reduce_partials3(partial, nblk, stride, out0, out1, out2, n, accumulate0, accumulate1, accumulate2,
                       (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_reduce_splits(const float* ws, int splits, size_t stride, int N1, int N2, float* out, int ldo, int accumulate,
                         sgl_stream stream) {
  if (!ws || !out) return SGL_ERR_NULL;
  if (splits <= 0 || N1 <= 0 || N2 <= 0 || ldo < N2 || (splits > 1 && stride < (size_t)N1 * N2)) return SGL_ERR_BAD_SHAPE;
  CKV(reduce_splits(ws, splits, stride, N1, N2, out, ldo, accumulate, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_add_f32(const float* a, const float* b, float* out, size_t n, sgl_stream stream) {
  if (!a || !out) return SGL_ERR_NULL;
  // copy_f32_kernel moves float4s without looking at the pointers
  if (!aligned16(a) || !aligned16(out) || (b && !aligned16(b))) return SGL_ERR_UNSUPPORTED;
  CKV(add_f32(a, b, out, n, (hipStream_t)stream));
  return SGL_OK;
}

int sgl_op_cast_f32(const float* src, void* dst, int dst_dtype, size_t n, sgl_stream stream) {
  if (!src || !dst) return SGL_ERR_NULL;
  if (!lo_dtype_ok(dst_dtype)) return SGL_ERR_UNSUPPORTED;
  CKV(cast_f32(src, dst, dst_dtype, n, (hipStream_t)stream));
  return SGL_OK;
}

}  // extern "C"
