/* siglip_hip.h — C ABI of libsiglip_hip.so: the MI355X (gfx950) SigLIP-2 vision-encoder hot path.
 *
 * The reference has no FFI of its own: its "plugin API" for this path is two Python call surfaces on an
 * nn.Module obtained from third-party libraries:
 *   surface H  self.encoder(pixel_values=..., output_hidden_states=True, interpolate_pos_encoding=True)
 *              -> .pooler_output / .last_hidden_state / .hidden_states        Siglip2sidafrozen.py:753,787-793
 *              (+ output_attentions=True -> .attentions / .pooling_attention: sgl_attention_probs below)
 *   surface O  backbone.encode_image(x) -> (B, D)                             cifake_binary_classifier.py:721,
 *                                                                             hidf_video_classifier.py:307
 * The entry points below are what a binding for that path binds instead of the HuggingFace / open_clip ViT:
 * plain pointers and sizes, caller-owned memory, the caller's HIP stream.  INTEGRATION.md shows the ctypes
 * stub.  Rules common to every call:
 *   - returns 0 (SGL_OK) or a negative sgl_status; never throws, aborts, prints, allocates device memory or
 *     synchronises the device; sgl_last_hip_error(ctx) holds the hipError_t behind SGL_ERR_HIP;
 *   - argument errors (SGL_ERR_NULL / BAD_SHAPE / UNSUPPORTED / WORKSPACE) are reported before any work is enqueued and
 *     before any buffer is touched (tests/test_abi_contract_host.py makes every such call on a machine without a device);
 *   - all pointers are device pointers on the current device unless stated; work is enqueued on `stream`;
 *   - re-entrant per ctx as long as the calls on one ctx are stream-ordered; no thread-local state (PyTorch runs
 *     backward on an autograd worker thread);
 *   - fp32 master parameters use the HuggingFace layouts (Linear W[out,in] row-major, patch conv W[D,3,p,p],
 *     nn.MultiheadAttention in_proj_weight [3D,D] in q,k,v order).
 */
#ifndef SIGLIP_HIP_H
#define SIGLIP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgl_ctx sgl_ctx;
typedef void* sgl_stream; /* hipStream_t */

enum { SGL_DTYPE_F32 = 0, SGL_DTYPE_BF16 = 1, SGL_DTYPE_BF16X3 = 2, SGL_DTYPE_F16 = 3, SGL_DTYPE_MXFP8 = 5 };
/* code 4 is not assigned: sgl_create rejects it like every other unknown code */
enum { SGL_DTYPE_U8 = 6 };   /* a STORAGE type only (the mask bytes sgl_op_seg_eval reads): never a compute dtype */

typedef enum {
  SGL_OK = 0,
  SGL_ERR_BAD_SHAPE = -1,   /* B <= 0, image smaller than one patch, too many tokens, a non-native grid without
                               interpolate_pos, hs_slots / layer out of range.  Rectangular grids (H / p, W / p) and
                               trailing pixels beyond the last whole patch are supported.
                               With use_head = 1 the pooling head limits the tokens of ONE image, N = (H / p) * (W / p),
                               with c = round_up(head_dim, 16) / 8: N <= floor(16376 / (c + 1)) for inference and
                               N <= floor(16376 / (c + 2)) for training (sgl_query_sizes(train = 1), a forward given
                               `saved`, every sgl_backward_*).  so400m (head_dim 72): 1488 / 1364 tokens, so the
                               largest square images are 532 px (inference) and 504 px (training), 546 / 518 px are
                               refused; base (head_dim 64): 1819 / 1637 tokens, 672 / 640 px pass, 688 / 656 px are
                               refused.  A context with use_head = 0 has no such limit */
  SGL_ERR_UNSUPPORTED = -2, /* dtype / config outside what the kernels implement */
  SGL_ERR_WORKSPACE = -3,   /* saved / workspace / shadow buffer smaller than sgl_query_sizes reports */
  SGL_ERR_HIP = -4,         /* a HIP call failed: see sgl_last_hip_error */
  SGL_ERR_NULL = -5         /* a required pointer is NULL (the layers tables of sgl_weights / sgl_grads and a workspace the
                               call needs included) */
} sgl_status;

/* Immutable model description (HF SiglipVisionConfig fields; TF:models/siglip/configuration_siglip.py:90-99). */
typedef struct {
  int hidden_size;        /* D */
  int intermediate_size;  /* I */
  int num_layers;         /* L */
  int num_heads;          /* H, head_dim = D / H must be a multiple of 8 and <= 96 */
  int patch_size;         /* p */
  int native_grid;        /* image_size / p : side of the stored position table */
  float layer_norm_eps;   /* 1e-6 */
  int compute_dtype;      /* SGL_DTYPE_BF16: bf16 MFMA operands, fp32 accumulate / residual stream / statistics;
                             SGL_DTYPE_F32 : strict fp32 everywhere (parity mode; plain fp32 FMAs, no matrix cores);
                             SGL_DTYPE_BF16X3: strict mode ON the matrix cores: activations, weights and buffers exactly as
                                in SGL_DTYPE_F32, but every GEMM runs as one bf16 MFMA GEMM over split operands
                                (x = hi + lo; hi*hi + hi*lo + lo*hi, fp32 accumulate: ~2^-17 relative per product) and
                                attention as fp32 MFMA; meets "logits within 1e-3" at a fraction of SGL_DTYPE_F32's cost;
                             SGL_DTYPE_F16 : SGL_DTYPE_BF16 with fp16 operands (fp16 MFMA, fp32 accumulate / residual stream /
                                statistics / softmax, fp16 weight shadows): the arithmetic of an fp16-autocast run, 3 more
                                mantissa bits than bf16 at the same MFMA rate; overflow of an fp16 operand gives +-inf;
                             SGL_DTYPE_MXFP8: INFERENCE ONLY.  The four projection GEMMs of every block (QKV, out_proj,
                                fc1, fc2) run on MX-fp8 operands (OCP e4m3fn elements, one E8M0 scale per 32 K-elements,
                                v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulate); everything else as SGL_DTYPE_BF16
                                (fp32 residual stream and statistics, bf16 attention, patch embedding and pooling head).
                                The weight shadows are MX blocks (re-quantized by sgl_prepare_weights*).  Training is
                                refused: sgl_query_sizes(train=1) and sgl_forward* with saved != NULL return
                                SGL_ERR_UNSUPPORTED, and sgl_adamw_bind_shadows binds nothing */
  int use_head;           /* attention-pool head present (vision_use_head) */
} sgl_config;

/* fp32 master parameters of one encoder block (TF:modeling_siglip.py:268-271,315-316,329-331). */
typedef struct {
  const float *ln1_w, *ln1_b;
  const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b;
  const float *ln2_w, *ln2_b;
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} sgl_layer_weights;

typedef struct {
  const float *patch_w, *patch_b; /* [D, 3*p*p], [D] */
  const float* pos;               /* [native_grid^2, D] */
  const sgl_layer_weights* layers; /* HOST array of num_layers entries (device pointers inside) */
  const float *post_ln_w, *post_ln_b;
  /* attention-pool head (TF:modeling_siglip.py:622-643); ignored when use_head == 0 */
  const float *probe;                     /* [D] */
  const float *in_proj_w, *in_proj_b;     /* [3D, D], [3D] */
  const float *out_proj_w, *out_proj_b;   /* [D, D], [D] */
  const float *head_ln_w, *head_ln_b;
  const float *head_fc1_w, *head_fc1_b, *head_fc2_w, *head_fc2_b;
} sgl_weights;

/* Gradient destinations, same layouts as sgl_weights.  A NULL pointer means "frozen: do not compute".
 * accumulate != 0 adds into the buffers (gradient accumulation), otherwise they are overwritten: every non-NULL
 * destination of a step that runs is written in full, with zeros where the gradient is identically zero (k_b always;
 * the pooling head without d_pooled; post_layernorm with neither d_pooled nor d_last_hidden). */
typedef struct {
  float *ln1_w, *ln1_b;
  float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b;
  float *ln2_w, *ln2_b;
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} sgl_layer_grads;

typedef struct {
  float *patch_w, *patch_b, *pos;
  const sgl_layer_grads* layers; /* HOST array of num_layers entries */
  float *post_ln_w, *post_ln_b;
  float *probe, *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *head_ln_w, *head_ln_b;
  float *head_fc1_w, *head_fc1_b, *head_fc2_w, *head_fc2_b;
  int accumulate;
} sgl_grads;

/* ---- lifetime ------------------------------------------------------------------------------------- */
sgl_ctx* sgl_create(const sgl_config* cfg); /* NULL if the config is unsupported */
/* Activation policy of a context (gradient checkpointing).  SGL_RECOMPUTE_NONE: a training forward keeps every block's
 * activations in `saved` until the backward.  SGL_RECOMPUTE_BLOCKS: it keeps only each block's input (the hidden states)
 * and sgl_backward_layer* recomputes the block; see "recompute context" below. */
enum { SGL_RECOMPUTE_NONE = 0, SGL_RECOMPUTE_BLOCKS = 1 };
/* sgl_create with an activation policy; sgl_create_ex(cfg, SGL_RECOMPUTE_NONE) is sgl_create(cfg).  NULL for any other
 * policy value, and for SGL_DTYPE_MXFP8 with SGL_RECOMPUTE_BLOCKS (that mode never trains). */
sgl_ctx* sgl_create_ex(const sgl_config* cfg, int recompute);
void sgl_destroy(sgl_ctx* ctx);
int sgl_last_hip_error(const sgl_ctx* ctx);
const char* sgl_status_string(int status);
int sgl_abi_version(void);

/* ---- sizes (bytes) for caller-allocated buffers ----------------------------------------------------- */
/* shadow: compute-dtype copies of the weight matrices (padded, plus pre-transposed forms for dX GEMMs);
 * saved:  activations kept from forward for backward (0 when train == 0);
 * ws:     scratch; must stay untouched between sgl_backward_begin and the last sgl_backward_* call.
 * Recompute context (sgl_create_ex(cfg, SGL_RECOMPUTE_BLOCKS)); every entry point keeps its signature and obeys it:
 *   - train == 1: `saved` holds no per-block region (it keeps the patch operand, the resized position table, the
 *     post-LayerNorm statistics and the pooling-head activations); `ws` is larger by ONE block region, which the training
 *     forward and every sgl_backward_layer* call reuse.  train == 0 sizes and the shadow size are those of a plain context;
 *   - a training forward (saved != NULL) also needs `ws` (ws_bytes of train == 1): it writes each block's activations into
 *     the shared region (the GELU pre-activation nowhere) and every hidden-state slot as on a plain context; nothing in
 *     `ws` has to survive from the forward to the backward;
 *   - sgl_backward_layer*(layer) first recomputes block `layer` from its input hidden state into the shared region (LN1,
 *     QKV, attention, out_proj + residual, LN2, fc1 + GELU; not fc2), then runs the plain backward of the block.  The call
 *     sequence and the gradient carried in `ws` between calls are unchanged.
 * Token limit (every context, plain and recompute, every pass): B * grid must not exceed floor((2^32 - 1) / R), R = the
 * bytes of one row of the widest GEMM operand of the pass, nor exceed 2^22 - 1 (the QKV scatter's row split).  The widest
 * row is max(round_up(I, 128), hidden_size, round_up(3 * p^2, 64)) elements at inference and max(that, 3 * hidden_size)
 * when training, of the compute dtype: two bytes in bf16 / fp16, four in fp32, 6 * round_up(that, 8) for the bf16x3 split
 * operand.  The GEMMs refuse an operand of 2^32 bytes.  MX-fp8: R = 2 * max(hidden_size, round_up(3 * p^2, 64)), the bf16
 * patch and head GEMMs it still runs, and at most 65 535 * 128 tokens (the MX GEMM's grid).  Larger shapes return
 * SGL_ERR_BAD_SHAPE from sgl_query_sizes, sgl_forward* and sgl_backward_* before anything is enqueued.  so400m: 493 447
 * tokens in bf16 / fp16 (B = 676 at 384 px), 246 723 in fp32, 164 482 in bf16x3, for inference and training alike (its
 * widest row is the MLP's 4352 on both); 1 864 135 in MX-fp8. */
int sgl_query_sizes(const sgl_ctx* ctx, int B, int H, int W, int train, size_t* shadow_bytes, size_t* saved_bytes,
                    size_t* ws_bytes);

/* Refresh the shadow arena from the fp32 masters (call after every optimizer step / load_state_dict).
 * Replaces the per-step autocast weight casts of the reference (Siglip2sidafrozen.py:1375). */
int sgl_prepare_weights(sgl_ctx* ctx, const sgl_weights* w, void* shadow, size_t shadow_bytes, sgl_stream stream);
/* Same, restricted to what changed since the last call: layer_dirty[l] != 0 re-casts block l (NULL = all blocks),
 * globals_dirty != 0 re-casts the patch-embedding and pooling-head matrices.  For frozen-prefix fine-tuning. */
int sgl_prepare_weights_dirty(sgl_ctx* ctx, const sgl_weights* w, void* shadow, size_t shadow_bytes,
                              const unsigned char* layer_dirty, int globals_dirty, sgl_stream stream);

/* ---- forward ---------------------------------------------------------------------------------------- */
/* pixels: fp32 (B,3,H,W) NCHW, or NHWC storage when channels_last == 1 (reference .to(channels_last),
 *         Siglip2sidafrozen.py:1191,1365).  Grid = (H / p, W / p) as in a "valid" conv (384 / 14 = 27).
 *         channels_last == 2: `pixels` is instead the ready patch-major operand [B*grid^2][round_up(3p^2,64)] in the
 *         compute dtype (sgl_op_preprocess, patch_major): the gather pass is skipped (H, W still give the geometry).
 * hidden_states: fp32 [hs_slots][B*N][D]; slot l holds hidden_states[l] of the HF output (0 = embeddings,
 *         L = last block output before post_layernorm).  hs_slots = L+1 keeps all of them (required when
 *         saved != NULL); hs_slots = 2 ping-pongs (inference without taps).
 * last_hidden: fp32 [B*N][D] (post_layernorm output).   pooled: fp32 [B][D] or NULL.
 * interpolate_pos != 0: bicubic-resize the position table when the grid differs from native
 *         (TF:modeling_siglip.py:137-173); with 0 the grid must equal the native grid. */
int sgl_forward(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const float* pixels, int channels_last, int B,
                int H, int W, int interpolate_pos, float* hidden_states, int hs_slots, float* last_hidden,
                float* pooled, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream);
/* sgl_forward with a frozen prefix declared: blocks < first_trainable_block will not be differentiated
 * (sgl_backward_layer is never called for them), so their GELU pre-activations are not saved.  A caller who wants the
 * input gradient (sgl_backward_embed_px) passes 0, whatever is frozen: the backward then runs through every block, and
 * the GELU pre-activations are saved for every block. */
int sgl_forward_ex(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const float* pixels, int channels_last, int B,
                   int H, int W, int interpolate_pos, float* hidden_states, int hs_slots, float* last_hidden,
                   float* pooled, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, int first_trainable_block,
                   sgl_stream stream);

/* sgl_forward_ex with one pointer per hidden-state slot (HOST array of L+1 device pointers, each [B*N][D] fp32) instead
 * of one [slots][B*N][D] block: the PyTorch custom op (torch.ops.siglip_hip.encoder_fwd) hands the requested taps out as
 * tensors of their own and keeps the other slots in a private buffer, so no output aliases another.  Inference callers
 * may point several entries at the same buffer (ping-pong) as long as slots l and l+1 differ; with saved != NULL all
 * L+1 pointers must be distinct. */
int sgl_forward_slots(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const float* pixels, int channels_last,
                      int B, int H, int W, int interpolate_pos, float* const* hs_slots, float* last_hidden,
                      float* pooled, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                      int first_trainable_block, sgl_stream stream);

/* ---- ragged batches: images of different sizes in one forward (new symbols; sgl_abi_version() stays 3) ------------------
 * Inference only: there is no `saved` argument, so training cannot be asked for.  Works in all five compute modes, on
 * plain and recompute contexts alike (inference on a recompute context equals a plain one).
 * Packed layout: the S images of a call have grids (gh_s, gw_s), grids = HOST int32 [S][2], and n_s = gh_s * gw_s tokens.
 *   Image s owns rows cu[s] .. cu[s+1]-1 of every token-major buffer, cu = the exclusive prefix sum of the n_s;
 *   T = cu[S] rows in all; max_n = the largest n_s.  There are no padding rows.
 * patches: the patch-major operand [T][round_up(3p^2, 64)] in the compute dtype (the channels_last == 2 form of
 *   sgl_forward); image s occupies its n_s rows in row-major patch order, as sgl_op_im2col writes them for B = 1.  It is
 *   only read.
 * hs_slots: HOST array of L+1 device pointers, each [T][D] fp32; ping-pong allowed as in sgl_forward_slots (slots l and
 *   l+1 must differ).  last_hidden: [T][D].  pooled: [S][D] or NULL.
 * The position table is always fitted to each image's grid (interpolate_pos != 0 of sgl_forward): the stored table for a
 * native grid, the bicubic resize otherwise.
 * Numerics: LayerNorm, the GEMMs and their epilogues and the MX quantiser work row by row, and the two attention stages run
 * sgl_op_attn_fwd_varlen / sgl_op_pool_attn_fwd_varlen (below), so every row of every output holds the bits that
 * sgl_forward_slots(B = 1, interpolate_pos = 1) gives the image alone.
 * ws: ws_bytes >= what sgl_query_sizes_ragged reports: the inference workspace of (B = 1, N = T) with S rows in the pooling
 *   head's per-image buffers, the packed position table [T][D] and, last, cu.  For S = 1 that is what
 *   sgl_query_sizes(B = 1, train = 0) reports for the image plus 256 bytes (cu); it never shrinks when T grows.
 * Errors, in this order, before anything is enqueued: a NULL pointer (ctx, w, shadow, patches, grids, hs_slots,
 *   last_hidden, ws, w->layers with L > 0) -> SGL_ERR_NULL; S < 1, a grid side < 1, T above the inference token limit of
 *   sgl_query_sizes, with the pooling head max_n above sgl_op_pool_attn_fwd's forward limit, or a max_n the context's
 *   attention route refuses for one image (strict fp32: its scores no longer fit the LDS) -> SGL_ERR_BAD_SHAPE; a NULL
 *   entry of hs_slots -> SGL_ERR_NULL; ws_bytes too small -> SGL_ERR_WORKSPACE.  sgl_query_sizes_ragged: ctx / grids NULL,
 *   then the same shape checks. */
int sgl_query_sizes_ragged(const sgl_ctx* ctx, const int* grids, int S, size_t* ws_bytes);
int sgl_forward_ragged(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const void* patches, const int* grids, int S,
                       float* const* hs_slots, float* last_hidden, float* pooled, void* ws, size_t ws_bytes,
                       sgl_stream stream);

/* ---- backward (stepwise so that a data-parallel caller can all-reduce each block's gradients while the
 *      next block's backward runs; sgl_backward is the plain loop over the three steps) ------------------ */
/* d_last_hidden [B*N][D], d_pooled [B][D], d_tap_last [B*N][D] (gradient w.r.t. hidden_states[L]); any may be
 * NULL.  Computes head + post_layernorm gradients and leaves d hidden_states[L] in the workspace. */
int sgl_backward_begin(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int B, int H, int W,
                       const float* hidden_states, const float* d_last_hidden, const float* d_pooled,
                       const float* d_tap_last, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                       sgl_stream stream);
/* Block `layer`: parameter gradients of that block, then workspace gradient := d hidden_states[layer]
 * (+ d_tap, the external gradient w.r.t. hidden_states[layer], may be NULL).  need_dx == 0 skips the input
 * gradient (first trainable block of a frozen prefix, Siglip2sidafrozen.py:762-768). */
int sgl_backward_layer(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int layer, int B,
                       int H, int W, const float* hidden_states, const float* d_tap, int need_dx, const void* saved,
                       size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream);
/* The same two steps taking just the hidden state they read (hidden_states[L] / hidden_states[layer]) instead of the
 * base of a contiguous [L+1][B*N][D] block: for callers that keep the slots in separate buffers (sgl_forward_slots). */
int sgl_backward_begin_p(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int B, int H, int W,
                         const float* hs_last, const float* d_last_hidden, const float* d_pooled,
                         const float* d_tap_last, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                         sgl_stream stream);
int sgl_backward_layer_p(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int layer, int B,
                         int H, int W, const float* hs_in, const float* d_tap, int need_dx, const void* saved,
                         size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream);
/* Patch-embedding / position-table gradients from the workspace gradient (d hidden_states[0]). */
int sgl_backward_embed(sgl_ctx* ctx, const sgl_weights* w, const sgl_grads* g, int B, int H, int W, int interpolate_pos,
                       const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream);
/* ---- gradient with respect to the input pixels (new symbols; sgl_abi_version() stays 3: nothing existing changed) ------
 * sgl_backward_embed_px does everything sgl_backward_embed does, for whichever of g->patch_w / patch_b / pos are non-NULL
 * (all three may be NULL: a frozen encoder), and then writes d_pixels = d loss / d pixels: fp32 (B,3,H,W), NCHW, or NHWC
 * storage when channels_last == 1 (the storage the forward read; 2, the ready patch operand, is SGL_ERR_UNSUPPORTED).
 * d_pixels is ALWAYS overwritten, every element of it: g->accumulate governs the parameter destinations only; the
 * trailing rows / columns of an image the patch size does not divide feed nothing and get exact zeros.
 * Call order: sgl_forward* with first_trainable_block = 0, sgl_backward_begin*, sgl_backward_layer* for EVERY block
 * L-1 ... 0 with need_dx = 1 (gradient destinations of frozen blocks NULL), then this call instead of sgl_backward_embed.
 * px_scratch: px_scratch_bytes >= what sgl_query_input_grad_bytes reports for (B, H, W): the patch GEMM's dX
 * [B*N][round_up(3p^2, 64)] fp32 and the transposed patch weight in the compute dtype, cast per call (the shadow arena has
 * no such copy and sgl_query_sizes reports what it always reported); the bf16x3 split of that one product fits the split
 * scratch `ws` already holds.  Needed only during the call.
 * Errors, all before anything is enqueued: the checks of sgl_backward_embed, plus d_pixels / px_scratch / w->patch_w NULL
 * -> SGL_ERR_NULL (first), px_scratch_bytes too small -> SGL_ERR_WORKSPACE (after the saved / ws checks); the token limit
 * of a recompute context applies (SGL_ERR_BAD_SHAPE); an SGL_DTYPE_MXFP8 context -> SGL_ERR_UNSUPPORTED from both. */
int sgl_query_input_grad_bytes(const sgl_ctx* ctx, int B, int H, int W, size_t* scratch_bytes);
int sgl_backward_embed_px(sgl_ctx* ctx, const sgl_weights* w, const sgl_grads* g, int B, int H, int W,
                          int interpolate_pos, float* d_pixels, int channels_last, void* px_scratch,
                          size_t px_scratch_bytes, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                          sgl_stream stream);
/* d_taps: HOST array of L+1 device pointers (NULL entries allowed) or NULL.  Stops above first_trainable_block.
 * (No input gradient: a caller who wants d_pixels makes the stepwise calls above.) */
int sgl_backward(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int B, int H, int W,
                 int interpolate_pos, const float* hidden_states, const float* const* d_taps,
                 const float* d_last_hidden, const float* d_pooled, int first_trainable_block, int train_embeddings,
                 const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream);

/* ---- single-kernel entry points (unit parity tests, micro-benchmarks, roofline measurement) ----------- */
int sgl_op_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                         float* rstd, int M, int D, float eps, sgl_stream stream);
int sgl_op_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* mean, const float* rstd,
                         const float* gamma, const float* dres, float* dx, void* dx_lp, int lp_dtype, float* dgamma,
                         float* dbeta, float* scratch, size_t scratch_bytes, int M, int D, sgl_stream stream);
/* epilogue selectors for sgl_op_gemm_nt */
enum { SGL_EPI_STORE = 0, SGL_EPI_BIAS_GELU = 1, SGL_EPI_RES_F32 = 2, SGL_EPI_QKV = 3, SGL_EPI_GELU_BWD = 4,
       SGL_EPI_POS_F32 = 5, SGL_EPI_F32 = 6 };
/* C[M,N] = A[M,K] * B[N,K]^T with a fused epilogue; dtype is the operand dtype (bf16 / fp16 -> MFMA kernel; the 16-bit
 * outputs of EPI_STORE / BIAS_GELU / QKV / GELU_BWD are in the operand dtype).
 * SGL_EPI_QKV (N = 3 * heads * head_dim, M = batch * tokens; ldo is not used) is the write side of the head-major layout
 *   sgl_op_attn_fwd reads with ld_qkv == 0, the one the encoder uses: column which * heads * head_dim + h * head_dim + d of
 *   row b * tokens + n goes to out[which][b][h][n][d] of [3][batch][heads][tokens][head_dim_pad], and the pad columns
 *   [head_dim, head_dim_pad) of every row are written as +0 (head_dim % 8 == 0, head_dim_pad % 8 == 0).  Every head's
 *   [tokens][head_dim_pad] matrix is contiguous; for 16-bit outputs with head_dim 72 / head_dim_pad 80 and heads % 4 == 0
 *   (so400m) the large-M kernel works on tiles of four whole heads and writes each head's rows as runs of whole rows.
 *   SGL_EPI_QKV with M >= 2^22 is refused (SGL_ERR_UNSUPPORTED, nothing written): the epilogue's row split (row / tokens by a
 *   reciprocal estimate and one correction) is exact for rows below 2^22 only.  A 16-bit operand of 2^32 bytes or more
 *   (M * lda * 2, N * ldb * 2) is refused the same way. */
int sgl_op_gemm_nt(int dtype, const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, void* out,
                   int ldo, void* out2, int ldo2, const float* bias, const float* res, int ldr, const void* aux,
                   int ldaux, const float* pos, int pos_rows, int tokens, int heads, int head_dim, int head_dim_pad,
                   int batch, sgl_stream stream);
/* MX-fp8 single-kernel entry points (the SGL_DTYPE_MXFP8 mode's kernels).  An MX operand [rows][Kp] is Kp e4m3fn bytes per
 * row plus E8M0 scale bytes [rows][Kp/32] (value = e4m3 * 2^(scale - 127)); Kp % 128 == 0, padding bytes and scales are 0.
 * Quantizer, per 32-block with amax = max|x|: e = the smallest integer with amax <= 448 * 2^e, clamped to [-127, 127];
 * scale byte e + 127; elements x * 2^-e rounded to nearest even (subnormals kept); an all-zero block has scale byte 0; a
 * block holding an inf or NaN gets scale byte 0xFF and NaN elements (0x7F).
 * sgl_op_quantize_mxfp8: x [M][K] (ldx elements, x_dtype SGL_DTYPE_F32 or SGL_DTYPE_BF16) -> q [M][Kp] + scales. */
int sgl_op_quantize_mxfp8(const void* x, int x_dtype, int ldx, int M, int K, int Kp, void* q, void* scales,
                          sgl_stream stream);
/* LayerNorm of x [M][D] (fp32 statistics, as sgl_op_layernorm_fwd) written as an MX operand [M][Kp] (D <= Kp <= 2048). */
int sgl_op_layernorm_fwd_mx(const float* x, const float* gamma, const float* beta, void* q, void* scales, int M, int D,
                            int Kp, float eps, sgl_stream stream);
/* C[M,N] = A[M,Kp] * B[N,Kp]^T on MX operands (A with scales As, B with scales Bs), fp32 accumulate, fused epilogue:
 * SGL_EPI_RES_F32 (fp32 out = res + acc + bias), SGL_EPI_QKV (bf16 head-major scatter, as sgl_op_gemm_nt) or
 * SGL_EPI_BIAS_GELU (gelu_tanh(acc + bias) quantized to an MX operand: out [M][ldo] bytes, out_scales [M][ldo/32];
 * N % 32 == 0, ldo % 128 == 0, columns N..ldo untouched).  bias is required. */
int sgl_op_gemm_nt_mx(const void* A, const void* As, const void* B, const void* Bs, int M, int N, int Kp, int epi,
                      void* out, int ldo, void* out_scales, const float* bias, const float* res, int ldr, int tokens,
                      int heads, int head_dim, int head_dim_pad, int batch, sgl_stream stream);
/* C[N1,N2] (+)= sum_m A[m,N1] * B[m,N2]  (fp32 output). */
int sgl_op_gemm_tn(int dtype, const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                   float* out, int ldo, int accumulate, sgl_stream stream);
/* Same with device scratch for the split-K partial tiles: with scratch >= splits_used * N1 * N2 * 4 bytes (64 MiB always
 * suffices for the 256x256-tile kernel) the splits are summed in a fixed order -> bitwise reproducible, no fp32 atomics. */
int sgl_op_gemm_tn_ws(int dtype, const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int splits,
                      float* out, int ldo, int accumulate, float* scratch, size_t scratch_bytes, sgl_stream stream);
/* Scaled-dot-product attention of one block (TF:modeling_siglip.py:227-247,288-301), all heads and images in one launch.
 * dtype: SGL_DTYPE_BF16 (bf16 operands, bf16 MFMA, fp32 softmax), SGL_DTYPE_F32 (fp32 operands, plain FMAs: the reference
 *   kernels), SGL_DTYPE_BF16X3 (fp32 operands on v_mfma_f32_32x32x2_f32: what the strict MFMA mode uses) or
 *   SGL_DTYPE_F16 (the bf16 kernels on fp16 operands, fp16 MFMA, fp32 softmax).
 * ld_qkv > 0 (the argument was added in ABI 3; an optional input layout, NOT the one the encoder uses): q, k, v point at
 *   the three column blocks of the QKV projection's token-major output [B*N][ld_qkv]; head h of token row r is the
 *   head_dim elements at r*ld_qkv + h*head_dim (16-byte aligned: head_dim % 8 == 0, ld_qkv % 8 == 0, pointers 16-byte
 *   aligned).  Nothing is padded in memory.
 * ld_qkv == 0 (what the encoder uses; DESIGN.md section 8.4 records the measurement behind that): head-major
 *   [B][H][N][head_dim_pad] matrices whose pad columns are zero (EPI_QKV's layout).
 * out: token-major [B*N][H*head_dim]; lse: [B][H][N]. */
int sgl_op_attn_fwd(int dtype, const void* q, const void* k, const void* v, void* out, float* lse, int B, int H, int N,
                    int head_dim, int head_dim_pad, int ld_qkv, sgl_stream stream);
/* dqkv: token-major [B*N][3*H*head_dim].  delta_scratch: 2 * B * H * N floats (per query and head the pair
 * {-lse * log2 e, -rowsum(dO * O) / sqrt(head_dim)}; ABI 1 took B * H * N floats here). */
int sgl_op_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* out, const void* dout,
                    const float* lse, void* dqkv, float* delta_scratch, int B, int H, int N, int head_dim,
                    int head_dim_pad, int ld_qkv, sgl_stream stream);
/* ---- attention maps (new symbols; sgl_abi_version() stays 3: nothing existing changed) --------------------------------
 * The attention probabilities of a block, recomputed from what a forward leaves behind: q, k head-major
 * [B][H][N][head_dim_pad] with zero pad columns (the ld_qkv == 0 layout above; 16-bit operands 16-byte aligned) and the
 * lse [B][H][N] sgl_op_attn_fwd wrote (natural log of the row sum of exp(q.k / sqrt(head_dim))).
 *   out[b,h,i,j] = exp2(S_ij * c - lse_i * log2 e),  c = log2 e / sqrt(head_dim)
 * which is the P the backward kernels differentiate: lse is used as given and rows are NOT renormalised.
 * mode SGL_ATTN_PROBS_FULL: out fp32 (B,H,N,N).  SGL_ATTN_PROBS_HEAD_MEAN: out fp32 (B,N,N), the mean over heads, summed in
 * ascending head order in registers (the per-head maps never exist in memory).  dtype as sgl_op_attn_fwd.  Every input is
 * const; every element of out is written by exactly one plain store (no atomics): two calls give the same bits.
 * Errors, before anything is enqueued: q / k / lse / out NULL -> SGL_ERR_NULL; a dimension < 1, head_dim > head_dim_pad
 * or a head_dim / head_dim_pad sgl_op_attn_fwd refuses for that dtype -> SGL_ERR_BAD_SHAPE; an unknown dtype or mode, or
 * misaligned 16-bit operands -> SGL_ERR_UNSUPPORTED. */
enum { SGL_ATTN_PROBS_FULL = 0, SGL_ATTN_PROBS_HEAD_MEAN = 1 };
int sgl_op_attn_probs(int dtype, const void* q, const void* k, const float* lse, float* out, int B, int H, int N,
                      int head_dim, int head_dim_pad, int mode, sgl_stream stream);
/* Attention maps of the encoder, read out of the activation arena `saved` that a saving forward (sgl_forward* with saved
 * != NULL) of the same (B, H, W) left on a plain context.  The arena is const here and stays bit-identical: a backward
 * may follow.  layer in [0, L): block `layer`, through sgl_op_attn_probs on the q, k, lse the block kept, with the
 * context's attention dtype; out fp32 (B,heads,N,N) (FULL) or (B,N,N) (HEAD_MEAN).  layer == L: the pooling head's probe
 * attention, from the probabilities its forward kept; out (B,heads,N) (FULL, a copy) or (B,N) (HEAD_MEAN, heads summed in
 * ascending order, then divided by heads).
 * Errors, in this order, before anything is enqueued: ctx / saved / out NULL -> SGL_ERR_NULL; a shape a training forward
 * refuses, or layer outside [0, L] -> SGL_ERR_BAD_SHAPE; a recompute context (it keeps no per-block q, k), an
 * SGL_DTYPE_MXFP8 context, layer == L without the head, or an unknown mode -> SGL_ERR_UNSUPPORTED; saved_bytes below what
 * sgl_query_sizes(train = 1) reports, or out_bytes below the result -> SGL_ERR_WORKSPACE. */
int sgl_attention_probs(sgl_ctx* ctx, int B, int H, int W, const void* saved, size_t saved_bytes, int layer, int mode,
                        float* out, size_t out_bytes, sgl_stream stream);
/* ---- gradient-weighted attention maps (new symbols; sgl_abi_version() stays 3: nothing existing changed) --------------
 * The gradient of a score with respect to the attention probabilities of a block, formed where the backward has every
 * operand: q, k, v head-major [B][H][N][head_dim_pad] with zero pad columns and lse [B][H][N] as sgl_op_attn_probs takes
 * them, and dout token-major [B*N][H*head_dim] in the operand dtype, exactly what sgl_op_attn_bwd takes.
 *   dP[b,h,i,j] = sum_d dout[b*N+i, h*head_dim+d] * v[b,h,j,d]      P = the expression of sgl_op_attn_probs
 *   kind SGL_ATTN_GRAD_DP: dP (what autograd leaves in `.grad` of an eager softmax);  SGL_ATTN_GRAD_PDP: P * dP;
 *   SGL_ATTN_GRAD_RELEVANCE: x > 0 ? x : (x != x ? x : 0) of x = P * dP, a relu that keeps a NaN.
 * mode SGL_ATTN_PROBS_FULL: out fp32 (B,H,N,N); SGL_ATTN_PROBS_HEAD_MEAN: out fp32 (B,N,N), heads summed in ascending
 * order in registers, one division by H.  dtype as sgl_op_attn_fwd.  Every input is const; every element of out is written
 * by exactly one plain store: two calls give the same bits.  A head reads its own head_dim columns of dout only: the
 * 16-byte chunk of a padded k-step that lies in the next head is read as zero, never multiplied by v's zero pad.
 * Errors, in the order and with the codes of sgl_op_attn_probs (v and dout join the NULL and alignment checks), plus an
 * unknown kind -> SGL_ERR_UNSUPPORTED; 16-bit operands also need N * H * head_dim * 2 < 2^31 (SGL_ERR_BAD_SHAPE). */
enum { SGL_ATTN_GRAD_DP = 0, SGL_ATTN_GRAD_PDP = 1, SGL_ATTN_GRAD_RELEVANCE = 2 };
int sgl_op_attn_grad_probs(int dtype, const void* q, const void* k, const void* v, const void* dout, const float* lse,
                           float* out, int B, int H, int N, int head_dim, int head_dim_pad, int kind, int mode,
                           sgl_stream stream);
/* The pooling head's form: da[b,h,n] = sum_d dout[b, h*head_dim+d] * V[b,h,n,d], combined with probs [B][H][N] by `kind`
 * as above; out fp32 (B,H,N) (FULL) or (B,N) (HEAD_MEAN).  V, probs, dout as sgl_op_pool_attn_bwd takes them (dtype
 * SGL_DTYPE_F32 / BF16 / F16, V 16-byte aligned, head_dim % 8 == 0, head_dim_pad % 8 == 0).  Errors: a NULL pointer ->
 * SGL_ERR_NULL; a dimension < 1 or an inconsistent head_dim -> SGL_ERR_BAD_SHAPE; an unknown dtype, kind or mode, or a
 * misaligned V -> SGL_ERR_UNSUPPORTED. */
int sgl_op_pool_attn_grad_probs(int dtype, const void* V, const float* probs, const float* dout, float* out, int B, int H,
                                int N, int head_dim, int head_dim_pad, int kind, int mode, sgl_stream stream);
/* A request to write one such map during a backward step.  out: fp32 device buffer of out_bytes >= the result. */
typedef struct {
  float* out;
  size_t out_bytes;
  int kind; /* SGL_ATTN_GRAD_* */
  int mode; /* SGL_ATTN_PROBS_* */
} sgl_attn_grad_req;
/* sgl_backward_layer_p / sgl_backward_begin_p with an optional request; req == NULL is exactly those functions.
 * sgl_backward_layer_pa: once the out_proj dX GEMM has written the gradient of the block's attention output, the map of
 * block `layer` is enqueued on the same stream from the block's saved q, k, v, lse with the context's attention dtype;
 * out (B,heads,N,N) or (B,N,N).  sgl_backward_begin_pa: the pooling head's map, once the gradient of its attention output
 * exists; out (B,heads,N) or (B,N).  Nothing but req->out is written, and every gradient and workspace byte the backward
 * produces is bit-identical with and without a request.
 * Errors of a request, after the argument and arena checks of the plain call and before anything is enqueued: req->out
 * NULL -> SGL_ERR_NULL; a recompute or SGL_DTYPE_MXFP8 context, the begin variant on a model without the head or without
 * d_pooled, or an unknown kind or mode -> SGL_ERR_UNSUPPORTED; the block variant at a (B, N) whose launch
 * sgl_op_attn_grad_probs refuses -> SGL_ERR_BAD_SHAPE; req->out_bytes below the result -> SGL_ERR_WORKSPACE. */
int sgl_backward_layer_pa(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int layer, int B,
                          int H, int W, const float* hs_in, const float* d_tap, int need_dx, const void* saved,
                          size_t saved_bytes, void* ws, size_t ws_bytes, sgl_stream stream,
                          const sgl_attn_grad_req* req);
int sgl_backward_begin_pa(sgl_ctx* ctx, const sgl_weights* w, const void* shadow, const sgl_grads* g, int B, int H, int W,
                          const float* hs_last, const float* d_last_hidden, const float* d_pooled,
                          const float* d_tap_last, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                          sgl_stream stream, const sgl_attn_grad_req* req);
int sgl_op_colsum(int dtype, const void* in, int ld, int M, int N, float* out, int accumulate, float* scratch,
                  size_t scratch_bytes, sgl_stream stream);
int sgl_op_im2col(const float* pixels, int channels_last, void* out, int out_dtype, int B, int H, int W, int P, int Kp,
                  sgl_stream stream);
/* The adjoint of sgl_op_im2col: d_cols fp32 [B*(H/P)*(W/P)][Kp] (columns k = c*P*P + ky*P + kx; columns >= 3*P*P are never
 * read and may hold anything) -> d_pixels fp32 (B,3,H,W), NCHW (channels_last == 0) or NHWC storage (1).  Patches do not
 * overlap: a pure gather, bitwise reproducible.  Every pixel is written; rows >= (H/P)*P and columns >= (W/P)*P get 0. */
int sgl_op_col2im(const float* d_cols, int B, int H, int W, int P, int Kp, float* d_pixels, int channels_last,
                  sgl_stream stream);
int sgl_op_pos_resize(const float* table, int native_grid, float* out, int gh, int gw, int D, sgl_stream stream);

/* ---- the kernels only the encoder calls (new symbols; sgl_abi_version() stays 3: nothing existing changed) -----------
 * These exist for tests and bindings: each is one launcher of csrc/kernels.h behind the argument checks below.  A NULL
 * required pointer is SGL_ERR_NULL (checked first), a non-positive or inconsistent dimension SGL_ERR_BAD_SHAPE, an
 * unknown dtype code, a pointer a vector access needs aligned and is not, or a launcher's own refusal
 * SGL_ERR_UNSUPPORTED; nothing is enqueued on a refusal.  dtype codes: SGL_DTYPE_F32 / BF16 / F16.
 *
 * Pooling-head attention, one query per head: q fp32 [H * head_dim] (shared by all images); K, V head-major
 * [B][H][N][head_dim_pad] of `dtype` with ZERO pad columns, 16-byte aligned; out [B][H * head_dim] of `dtype`; probs
 * fp32 [B][H][N].  head_dim % 8 == 0, head_dim_pad % 8 == 0.  One workgroup per (image, head) holds its partials in the
 * default 64 KiB LDS window: N <= floor(16376 / (head_dim_pad / 8 + 1)) forward and floor(16376 / (head_dim_pad / 8 + 2))
 * backward (head_dim_pad 80: 1488 / 1364; 64: 1819 / 1637), SGL_ERR_UNSUPPORTED above. */
int sgl_op_pool_attn_fwd(int dtype, const float* q, const void* K, const void* V, void* out, float* probs, int B, int H,
                         int N, int head_dim, int head_dim_pad, sgl_stream stream);
/* ---- ragged (varlen) kernels (new symbols; sgl_abi_version() stays 3) ---------------------------------------------------
 * Packed layout as sgl_forward_ragged: segment s = rows cu[s] .. cu[s+1]-1, cu a DEVICE int32 [S+1] table (what
 * sgl_op_seg_offsets writes), T rows in all, max_n >= the longest segment (a larger max_n changes no bit, only the launch).
 * sgl_op_attn_fwd_varlen: q, k, v head-major [H][T][head_dim_pad] with zero pad columns (the ld_qkv == 0 layout at B = 1,
 *   N = T); out token-major [T][H * head_dim]; lse [H][T]; dtype as sgl_op_attn_fwd, all four routes.  The launch covers
 *   S * H (segment, head) pairs times ceil(max_n / 128) query blocks (the strict fp32 route: ceil(max_n / 4)); a workgroup
 *   whose first query row lies past its segment exits.  Query blocks and key tiles start at the segment's first row and the
 *   fetches are bounded to the segment's rows (rows past n_s read as zeros, never as the neighbour's rows), so segment s gets,
 *   bit for bit, the out and lse of sgl_op_attn_fwd(B = 1, N = n_s, ld_qkv = 0) on its rows alone.
 * sgl_op_pool_attn_fwd_varlen: q, K, V as sgl_op_pool_attn_fwd with K, V [H][T][head_dim_pad]; out [S][H * head_dim];
 *   probs [H][T]; one workgroup per (segment, head), its LDS window sized by max_n: max_n above the forward limit of
 *   sgl_op_pool_attn_fwd is SGL_ERR_UNSUPPORTED.  Segment s gets the bits of sgl_op_pool_attn_fwd(B = 1, N = n_s).
 * Clamp contract: the kernels use lo = clamp(cu[s], 0, T), hi = clamp(cu[s+1], lo, T) and n_s = min(hi - lo, max_n).  A
 *   wrong table gives wrong numbers; it cannot make a kernel read or write outside the buffers as sized by T, S and H.
 * Errors, before anything is enqueued: a NULL pointer -> SGL_ERR_NULL; a dimension < 1, head_dim > head_dim_pad, or a
 *   (max_n, head_dim, head_dim_pad) that sgl_op_attn_fwd refuses for an image of max_n tokens -> SGL_ERR_BAD_SHAPE; an
 *   unknown dtype or misaligned 16-bit operands -> SGL_ERR_UNSUPPORTED.
 * sgl_op_seg_offsets: cu[i] = lens[0] + ... + lens[i-1] for i = 0 .. S from HOST lengths.  The sums travel by value in the
 *   arguments of a small kernel, 256 per launch: no copy from host memory, no allocation, no synchronisation, the caller's
 *   stream only, so it may be captured into a graph.  lens / cu NULL -> SGL_ERR_NULL; S < 1, a negative length or a total
 *   above 2^31 - 1 -> SGL_ERR_BAD_SHAPE. */
int sgl_op_attn_fwd_varlen(int dtype, const void* q, const void* k, const void* v, void* out, float* lse, const int* cu,
                           int S, int T, int max_n, int H, int head_dim, int head_dim_pad, sgl_stream stream);
int sgl_op_pool_attn_fwd_varlen(int dtype, const float* q, const void* K, const void* V, void* out, float* probs,
                                const int* cu, int S, int T, int max_n, int H, int head_dim, int head_dim_pad,
                                sgl_stream stream);
int sgl_op_seg_offsets(const int* lens, int S, int* cu, sgl_stream stream);
/* probs as written by the forward, dout fp32 [B][H * head_dim] -> dkv token-major [B * N][2 * H * head_dim] of `dtype`
 * (dK block, then dV block; 16-byte aligned; every element written) and dq_partial fp32 [B][H * head_dim] (the per-image
 * gradient of q, summed over images by the caller). */
int sgl_op_pool_attn_bwd(int dtype, const float* q, const void* K, const void* V, const float* probs, const float* dout,
                         void* dkv, float* dq_partial, int B, int H, int N, int head_dim, int head_dim_pad,
                         sgl_stream stream);
/* The transpose of sgl_op_pos_resize: dtable [native_grid^2][D] += R^T dout, dout [gh * gw][D].  ADDS into dtable; a
 * gather in a fixed order, bitwise reproducible. */
int sgl_op_pos_resize_bwd(const float* dout, int gh, int gw, float* dtable, int native_grid, int D, sgl_stream stream);
/* dst [Rp][Cp] (row stride ldd) = src [R][C] (fp32, row stride lds) rounded to nearest, zero outside R x C. */
int sgl_op_cast_pad(const float* src, int R, int C, int lds, void* dst, int dst_dtype, int Rp, int Cp, int ldd,
                    sgl_stream stream);
/* All weight shadows of one transformer block in one launch: up to 6 matrices (the row-major padded copy dst [Rp][Cp],
 * row stride ldd, and / or the transposed copy dst_t [Cp][Rp], row stride ldt; either may be NULL) and up to 4 fp32
 * vectors (dst[i] = i < n ? src[i] : 0 for i < np).  More than 6 / 4 is SGL_ERR_BAD_SHAPE. */
typedef struct {
  const float* src;
  void* dst;
  void* dst_t;
  int R, C, lds, Rp, Cp, ldd, ldt;
} sgl_cast_mat;
typedef struct {
  const float* src;
  float* dst;
  int n, np;
} sgl_cast_vec;
int sgl_op_cast_job(const sgl_cast_mat* mats, int nmat, const sgl_cast_vec* vecs, int nvec, int dst_dtype,
                    sgl_stream stream);
/* The operand split of SGL_DTYPE_BF16X3: hi = bf16(x), lo = bf16(x - hi), Cs = round_up(C, 8), zeros in columns C..Cs.
 * stacked == 0: dst [R][3 * Cs] bf16, row = [hi | hi | lo] (b_side 0) or [hi | lo | hi] (b_side 1);
 * stacked == 1: dst [3 * R][Cs] bf16, planes  hi, hi, lo  (b_side 0) or  hi, lo, hi  (b_side 1).  dst 16-byte aligned. */
int sgl_op_split3(const float* src, int R, int C, int ld, void* dst, int Cs, int b_side, int stacked, sgl_stream stream);
/* out[j] (+)= sum_b in[b * n + j], j < n. */
int sgl_op_batch_sum(const float* in, int B, size_t n, float* out, int accumulate, sgl_stream stream);
/* out[j] (+)= sum_i v[i] * W[i * cols + j]; scratch: 16 * cols floats (SGL_ERR_WORKSPACE below that). */
int sgl_op_vecmat(const float* v, const float* W, int rows, int cols, float* scratch, size_t scratch_bytes, float* out,
                  int accumulate, sgl_stream stream);
/* out[j] (+)= sum_b partial[b * stride + j], j < n, in a fixed order. */
int sgl_op_reduce_partials(const float* partial, int nblk, int stride, float* out, int n, int accumulate,
                           sgl_stream stream);
/* out_k[j] (+)= sum_b partial[b * stride + k * n + j] for k = 0, 1, 2 in one launch; a NULL output is skipped. */
int sgl_op_reduce_partials3(const float* partial, int nblk, int stride, float* out0, float* out1, float* out2, int n,
                            int accumulate0, int accumulate1, int accumulate2, sgl_stream stream);
/* out[r * ldo + c] (+)= sum_s ws[s * stride + r * N2 + c] in a fixed order.  N2, ldo and stride multiples of 4, out and ws
 * 16-byte aligned: SGL_ERR_UNSUPPORTED otherwise. */
int sgl_op_reduce_splits(const float* ws, int splits, size_t stride, int N1, int N2, float* out, int ldo, int accumulate,
                         sgl_stream stream);
/* out[i] = a[i] + b[i] (b NULL: a copy), i < n; a, b and out 16-byte aligned (SGL_ERR_UNSUPPORTED otherwise). */
int sgl_op_add_f32(const float* a, const float* b, float* out, size_t n, sgl_stream stream);
/* dst[i] = src[i] rounded to nearest in dst_dtype. */
int sgl_op_cast_f32(const float* src, void* dst, int dst_dtype, size_t n, sgl_stream stream);

/* ---- SID mask-decoder tail ---------------------------------------------------------------
 * Depthwise 3x3 convolution, zero padding 1, of SegFormerStrongDecoder's per-tap smoothing block
 * (nn.Conv2d(E, E, 3, padding=1, groups=E), Siglip2sidafrozen.py:713-718) on channels-last (B, gh, gw, E) data of
 * dtype f32 or bf16.  w9 holds the nine taps TAP-MAJOR in fp32: w9[k*E + e] = Conv2d.weight[e][0][k/3][k%3].
 * flip = 1 applies the 180-degree rotated taps (the data gradient: dx = sgl_op_dwconv3x3(dy, w9, NULL, flip = 1)).
 * E % 8 == 0 (bf16) / E % 4 == 0 (f32), E <= 1024, 256 % (E / 8 or 4) == 0.  x, y, w9 and bias (when not NULL) must be
 * 16-byte aligned (16-byte vector accesses); anything else is SGL_ERR_BAD_SHAPE, before any launch. */
int sgl_op_dwconv3x3(const void* x, int dtype, const float* w9, const float* bias, void* y, int B, int gh, int gw, int E,
                     int flip, sgl_stream stream);
/* dw10[k*E + e] (+)= sum over pixels of x(shifted by tap k) * dy for k < 9, and dw10[9*E + e] (+)= sum dy (the bias
 * gradient); two deterministic stages, scratch >= sgl_op_dwconv3x3_wgrad_scratch_bytes().  x and dy must be 16-byte
 * aligned (SGL_ERR_BAD_SHAPE otherwise, before any launch); dw10 and scratch need only their natural 4-byte alignment. */
size_t sgl_op_dwconv3x3_wgrad_scratch_bytes(int B, int gh, int gw, int E);
int sgl_op_dwconv3x3_wgrad(const void* x, const void* dy, int dtype, float* dw10, int accumulate, float* scratch,
                           size_t scratch_bytes, int B, int gh, int gw, int E, sgl_stream stream);

/* ---- GPU input pipeline (first slice) ----------------------------------------------------------
 * K.Resize(S, antialias=True) -> [MixUp] -> K.Normalize(mean, std) of the reference's per-batch GPU transform
 * (cifake_binary_classifier.py:1791-1794,812-817), optionally fused with the patch gather of the patch-embedding
 * convolution: src is uint8 NHWC (B,Hs,Ws,3) decoded bytes (src_is_u8_nhwc != 0, scaled by 1/255) or float32 NCHW
 * (B,3,Hs,Ws) in [0,1]; the image is resampled to S x S with torch's antialiased bilinear filter
 * (upsample_bilinear2d(antialias=True)); mix_index != NULL blends image b with image mix_index[b] (device int32[B]):
 * lam*img[b] + (1-lam)*img[mix_index[b]].
 *   patch_major != 0: out is the patch GEMM's A operand [B*(S/P)^2][Kp] in out_dtype (k = c*P*P + ky*P + kx, columns
 *                     >= 3*P*P zero), Kp as the encoder uses it (round_up(3*P*P, 64)): pass it to sgl_forward_slots with
 *                     channels_last = 2 and the im2col pass is skipped;
 *   patch_major == 0: out is (B,3,S,S) NCHW in out_dtype (the tensor the reference's transform returns). */
int sgl_op_preprocess(const void* src, int src_is_u8_nhwc, int B, int Hs, int Ws, void* out, int out_dtype, int S, int P,
                      int Kp, int patch_major, float mean, float std, const int* mix_index, float lam,
                      sgl_stream stream);
/* The adjoint of sgl_op_preprocess(patch_major = 0) for a float source: d_out fp32 (B,3,S,S) NCHW, the gradient with
 * respect to the transform's output -> d_src fp32 (B,3,Hs,Ws) NCHW, the gradient with respect to the source,
 *   d_src[b] = Wy^T (lam * d_out[b] + (1 - lam) * sum over {j : mix_index[j] == b} of d_out[j]) Wx / std
 * (mix_index == NULL: Wy^T d_out[b] Wx / std) with the fp32 filter weights the forward applies; mean does not enter.
 * mix_index (device int32[B]) need not be a permutation: an image may be referenced by several others, by itself or by
 * none.  The transform is linear, so no source values are needed; for a uint8 source the result is the gradient with
 * respect to the byte scaled to [0,1] (byte / 255).  A gather: d_src is always overwritten, every element, by one plain
 * store, with a fixed summation order and no atomics: bitwise reproducible.
 * scratch: sgl_op_preprocess_bwd_scratch_bytes() bytes of device memory, 4-byte aligned, for the per-axis filter tables a
 * pre-pass writes (0 bytes, and scratch may be NULL, when Hs == S and Ws == S: the forward's copy shortcut).
 * Refused before anything is enqueued, d_src untouched: d_out or d_src NULL (or scratch NULL when bytes are needed)
 * SGL_ERR_NULL; std == 0 or a dimension < 1 SGL_ERR_BAD_SHAPE; Hs > 16 * S or Ws > 16 * S SGL_ERR_UNSUPPORTED (the
 * forward's limit); scratch_bytes too small SGL_ERR_WORKSPACE. */
size_t sgl_op_preprocess_bwd_scratch_bytes(int B, int Hs, int Ws, int S);
int sgl_op_preprocess_bwd(const float* d_out, int B, int Hs, int Ws, int S, float std, const int* mix_index, float lam,
                          float* d_src, void* scratch, size_t scratch_bytes, sgl_stream stream);

/* ---- test-time views (new symbols; sgl_abi_version() stays 3: nothing existing changed) -------------------------------
 * The app's inference-side windows (appv3.py:3214-3250 detect_core, :3315 make_multicrops, :3381 compute_patch_grid):
 * V views of B same-size sources (layouts as sgl_op_preprocess) in one pass (the adjoint of the NCHW layout with respect
 * to a float source is sgl_op_preprocess_views_bwd below; the patch-operand layout is inference only).  A view is
 * an integer crop box, an optional quarter turn and an optional mirror; the result is resized to S x S, normalised and
 * stored as out[v][c][y][x] (patch_major == 0) or as the patch GEMM's operand rows out[(v*g + gy)*g + gx][k]
 * (patch_major != 0, g = S / P, columns >= 3*P*P exactly zero): sgl_op_preprocess's two layouts with b = v.
 *
 * Record constraints: 0 <= src < B; 0 <= x0 < x1 <= Ws and 0 <= y0 < y1 <= Hs (half-open, as PIL's crop);
 * turns in 0..3, counter-clockwise quarter turns (PIL's sign); keep_canvas and flip in {0, 1}.
 * With C the crop (h x w), the oriented image O is
 *   1. turns == 0: O = C;
 *   2. turns > 0, keep_canvas == 0: O = C rotated exactly (numpy.rot90(C, turns); PIL transpose(ROTATE_90) applied
 *      `turns` times; rotate(expand=True)): the extents swap for odd turns;
 *   3. turns > 0, keep_canvas == 1: O = what PIL's C.rotate(90 * turns) returns with its defaults (expand=False, nearest,
 *      fill 0), the reference's rotated view.  The canvas stays h x w.  For turns == 2, or when w == h, this is the exact
 *      rotation; otherwise the centre part of the rotated crop is kept and the rest is zero:
 *        turns == 1:  O[y][x] = C[x + ((h - w + 1) >> 1)][((w + h - 1) >> 1) - y]
 *        turns == 3:  O[y][x] = C[((w + h - 1) >> 1) - x][y + ((w - h + 1) >> 1)]
 *      where the indices fall inside C, zero elsewhere (>> is the arithmetic shift: floor).  When w - h is odd the centre
 *      falls on half pixels and this truncation decides which columns are kept: a w = 8, h = 5 crop at one turn gives
 *      O[y][x] = C[x - 1][6 - y] for x in 1..5 and zero for x in {0, 6, 7}.  Zero is pixel value 0 in [0, 1], so
 *      -mean / std after normalisation;
 *   4. flip == 1: O mirrored left-right (after the turn).
 * O is then resized to S x S with the arithmetic of sgl_op_preprocess (torch's antialiased triangle filter, `in` = O's
 * extents) and normalised as (v - mean) / std.  The kernel runs the same filter code, so the full-frame view
 * (0, 0, Ws, Hs) without turn or flip equals sgl_op_preprocess on the same source bit for bit, and a plain crop equals
 * sgl_op_preprocess on the contiguous cropped copy bit for bit, in both layouts and every output dtype.
 *
 * views is a HOST pointer (read during the call, not afterwards; the records reach the device by value in the kernel
 * arguments, 64 per launch: no allocation, no synchronisation, no copy, the caller's stream only, graph-capturable).
 * scratch: sgl_op_preprocess_views_scratch_bytes() bytes of device memory; this design needs none (0; scratch may be NULL).
 * Refused before anything is enqueued, out untouched: src, views or out NULL -> SGL_ERR_NULL; V <= 0, a record outside
 * the constraints above, or sgl_op_preprocess's shape rules (dimensions >= 1, std != 0, patch_major: P >= 1, S >= P,
 * Kp >= 3*P*P) -> SGL_ERR_BAD_SHAPE; an out_dtype other than F32 / BF16 / F16 -> SGL_ERR_UNSUPPORTED; an oriented extent
 * above 16 * S on either axis (the tap-length cap of sgl_op_preprocess) -> SGL_ERR_UNSUPPORTED; scratch_bytes below the
 * reported size -> SGL_ERR_WORKSPACE.
 * Deviations from the app, stated: PIL rounds to 8 bits after each resize pass and this path does not (within
 * 1.05 / 255 of PIL's BILINEAR resize on uint8 sources); the MAX_SIDE pre-shrink stays on the host (the frequency
 * features, extract_freq_vector, are sgl_op_freq_features below); the sources of one call share one size (ragged
 * batches: one call per size). */
typedef struct sgl_view {
  int32_t src, x0, y0, x1, y1, turns, keep_canvas, flip;
} sgl_view;
size_t sgl_op_preprocess_views_scratch_bytes(int V, int S);
int sgl_op_preprocess_views(const void* src, int src_is_u8_nhwc, int B, int Hs, int Ws, const sgl_view* views, int V,
                            void* out, int out_dtype, int S, int P, int Kp, int patch_major, float mean, float std,
                            void* scratch, size_t scratch_bytes, sgl_stream stream);
/* The adjoint of sgl_op_preprocess_views(patch_major = 0) for a float source (new symbols; sgl_abi_version() stays 3):
 * d_out fp32 (V,3,S,S), the gradient with respect to the views -> d_src fp32 (B,3,Hs,Ws) NCHW, the gradient with respect
 * to the sources (for a uint8 source: with respect to byte / 255).  With A_v the linear part of view v (crop, orient,
 * resize with the fp32 filter weights the forward applies),
 *   d_src[b] = (sum over {v : views[v].src == b} of A_v^T d_out[v]) / std;
 * mean does not enter, and the zero fill of a kept canvas receives no gradient.  The patch-operand layout has no adjoint.
 * A gather: every source element has one owning thread (which owns the three channels of its pixel) that sums, view
 * index ascending (then oy, then ox), the terms of every view whose box holds it, then multiplies by 1 / std once.  No atomics; every element of d_src is written by a plain
 * store, exactly 0 where no view covers it and for a source no view names; two calls on the same inputs give the same
 * bits.  views is a HOST pointer read during the call only; the records reach the device by value in the kernel
 * arguments, 64 per launch.  For V > 64 the first launch stores its partial sum and every later one loads it, goes on
 * adding and stores it again, in stream order: the bits do not depend on where the chunks end.  The caller's stream only,
 * no allocation, no copy, no host synchronisation: graph-capturable.
 * scratch: sgl_op_preprocess_views_bwd_scratch_bytes(views, V, S) bytes of device memory, 4-byte aligned: per view that
 * is not an S x S copy, the filter of every output index and the output range of every oriented row and column
 * (2 * S * 20 + (oh + ow) * 8 bytes; the size follows the oriented extents, hence the records), written by a pre-pass
 * launch in front of each gather launch.  The size function returns 0 for NULL views or V, S < 1.
 * Refused before anything is enqueued, d_src untouched: d_out, views or d_src NULL (or scratch NULL when bytes are
 * needed) SGL_ERR_NULL; V <= 0, a dimension < 1, std == 0 or a record outside the constraints of sgl_view
 * SGL_ERR_BAD_SHAPE; an oriented extent above 16 * S SGL_ERR_UNSUPPORTED; scratch_bytes too small SGL_ERR_WORKSPACE. */
size_t sgl_op_preprocess_views_bwd_scratch_bytes(const sgl_view* views, int V, int S);
int sgl_op_preprocess_views_bwd(const float* d_out, int B, int Hs, int Ws, const sgl_view* views, int V, int S, float std,
                                float* d_src, void* scratch, size_t scratch_bytes, sgl_stream stream);

/* ---- frequency / SRM feature vectors (new symbols; sgl_abi_version() stays 3: nothing existing changed) ----------------
 * The app's 24 numbers per window (appv3.py:1618-1728 extract_freq_vector, DETECT_USE_CLAHE off), which detect_core feeds
 * FreqMLP for each of its 9 crops and each grid cell: V windows onto B same-size uint8 NHWC sources in one pass,
 * inference only.  A window is an sgl_view with turns == keep_canvas == flip == 0 (the app takes these features from
 * unrotated windows only).  out is V x 24 floats; per view, in this order:
 *   a. the gray plane, bit for bit PIL's crop(box).convert("L").resize((256, 256), BICUBIC):
 *      L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16, then PIL's two uint8 passes, horizontal then vertical: bicubic
 *      a = -0.5, support = 2 * max(in / 256, 1), taps clamped to the box (nothing outside it is read), weights
 *      normalised by their sequential sum in double, converted to 22-bit fixed point rounding half away from zero, each
 *      pass clip8((sum k p + 2^21) >> 22).  The coefficients are computed on the device, one output index per thread, in
 *      fp64 with contraction off (add, mul, div only: IEEE-exact, so they are PIL's integers);
 *   b. exact-integer statistics of that plane: the three SRM kernels (zero padding k / 2, normalised by abs-sum + 1e-6)
 *      give integers times 1 / (255 abs-sum), the two db1 levels (2 x 2 blocks, factor 1/2; cH along height, cV along
 *      width, cD both) integers times 1 / 510 and 1 / 1020; sum n .. n^4 and the eight sum c^2 are taken in 64-bit
 *      integers, the central moments in 128-bit integers, then mean, population variance, kurtosis m4 / (v + 1e-6)^2 and
 *      mean |c|^2 in double;
 *   c. the 256 x 256 FFT of plane / 255, transformed in fp64 (twiddles from a table made in double) and rounded to fp32
 *      bin by bin, so that a bin's error is its own rounding and not a fraction of the DC term's; from the fp32 |F| and
 *      angle(F) over the fftshift-ed plane: the band sums El, Em, Eh (ratios to their total + 1e-6, and
 *      (Eh + 1e-6) / (El + 1e-6)), the
 *      least-squares slope over bucket index 0..38 of the bucket means of log(|F| + 1e-6) (empty buckets count as 0), the
 *      entropy of the 50-bin histogram of the phase over [-pi, pi] (the maximum joins the last bin; the app's fp32
 *      formula with its 1e-6 terms), and the population variance of the 8 sector means of |F|;
 *   d. the 24 values 7 spectral, 8 wavelet, 9 SRM; with standardize != 0, (v - mean) / (std + 1e-6) of the fp32 vector
 *      with the unbiased std, all zeros when std < 1e-6.
 * geometry: DEVICE pointer to 3 x 256 x 256 bytes, the band (0..2), bucket (0..38) and sector (0..7) index of every pixel
 * of the fftshift-ed plane, 255 = member of none (the DC pixel's bucket, the atan2 == pi half-row's sector).  The caller
 * builds them once with the app's own torch calls and keeps them (preprocess.freq_geometry); the kernels only reduce.
 * This argument is the one addition to the signature first proposed for this entry: a call that allocates nothing and
 * copies nothing cannot own 192 KiB of device tables.
 * All floating sums have a fixed order (no float atomics; integer atomics for the histogram and the integer sums): two
 * calls give the same bits.  gray_out, when not NULL, receives the V gray planes (V x 256 x 256 bytes).
 * views is a HOST pointer read during the call; records reach the device in the kernel arguments, 64 per launch group
 * (seven launches per 64 views).  scratch: sgl_op_freq_features_scratch_bytes() bytes of device memory, owned by the caller,
 * 16-byte aligned (SGL_ERR_UNSUPPORTED otherwise), contents undefined before and after.  No allocation, no
 * synchronisation, the caller's stream only.
 * Refused before anything is enqueued, out and gray_out untouched: src, views, geometry, out (or a needed scratch) NULL
 * -> SGL_ERR_NULL; B, Hs, Ws or V <= 0, src outside the batch, an empty box or one outside the source ->
 * SGL_ERR_BAD_SHAPE; a view with turns, keep_canvas or flip set, or a window side above 4096 (the resize stays within
 * 65 taps) -> SGL_ERR_UNSUPPORTED; scratch_bytes below the reported size -> SGL_ERR_WORKSPACE.
 * Not covered: CLAHE, float sources, a backward pass, the app's optional forensic detectors. */
size_t sgl_op_freq_features_scratch_bytes(int V, int Hs, int Ws);
int sgl_op_freq_features(const void* src_u8_nhwc, int B, int Hs, int Ws, const sgl_view* views, int V,
                         const unsigned char* geometry, float* out /* V x 24 */, int standardize,
                         unsigned char* gray_out /* V x 256 x 256 or NULL */, void* scratch, size_t scratch_bytes,
                         sgl_stream stream);

/* Augmentation branch of the video trainer's GPU transform (hidf_video_classifier.py:2868-2874): K.Resize(S, antialias) ->
 * RandomHorizontalFlip -> RandomRotation(+-5 deg, bilinear, zeros outside) -> ColorJitter -> K.Normalize, one pass, same
 * sources / outputs as sgl_op_preprocess.  Random draws stay with the caller: aug is a DEVICE table of B samples.
 *   flip != 0: mirror x.  (cos_a, sin_a): rotation about the image centre, counter-clockwise positive; (1, 0) = none.
 *   order[]: permutation of {0 brightness (x*f), 1 contrast ((x-m)*f+m, m = mean grey level of the image at that point),
 *   2 saturation ((x-grey)*f+grey), 3 hue (h += hue, fraction of the circle)}, each result clamped to [0,1];
 *   order[0] < 0 = no colour jitter for this sample.  grey_mean: device scratch of B floats.
 * kornia itself is not installed in the build image: parity with it is unpinned; oracle/preprocess_oracle.py restates
 * exactly the operators above (torchvision's definitions). */
typedef struct sgl_aug_sample {
  float flip, cos_a, sin_a, brightness, contrast, saturation, hue;
  int order[4];
  int reserved;
} sgl_aug_sample;
int sgl_op_preprocess_aug(const void* src, int src_is_u8_nhwc, int B, int Hs, int Ws, void* out, int out_dtype, int S,
                          int P, int Kp, int patch_major, float mean, float std, const sgl_aug_sample* aug,
                          float* grey_mean, sgl_stream stream);
/* The adjoint of sgl_op_preprocess_aug(patch_major = 0) with respect to its source (new symbols; sgl_abi_version() stays
 * 3, sgl_aug_sample is unchanged): d_out fp32 (B,3,S,S) NCHW, the gradient with respect to the transform's output ->
 * d_src fp32 (B,3,Hs,Ws) NCHW, the gradient with respect to a float source (for a uint8 NHWC source: with respect to
 * byte / 255; the result is NCHW either way).  The transform is not linear (clamps, the contrast step's per-image mean,
 * RGB <-> HSV), so the call takes the source and the records the forward had.  Nothing of the forward is saved: per
 * output pixel the resized, mirrored and rotated RGB and the colour chain are recomputed with the forward's own
 * arithmetic, and the chain is walked back: brightness f g [0 <= x f <= 1]; contrast, with ghat = g [0 <= u <= 1],
 * c ghat + (1 - c) w (sum of ghat over the image's pixels and channels) / S^2, w = (0.299, 0.587, 0.114); saturation
 * s ghat + (1 - s) w (sum of ghat over the pixel's channels); hue, the vector-Jacobian product of the operator above line
 * by line; then the transpose of the rotation's bilinear taps (taps outside the image dropped), the mirror undone, and
 * the resize adjoint of sgl_op_preprocess_bwd (tables, copy shortcut), where 1 / std is applied, once.  mean does not
 * enter.  Where the forward is not differentiable the result is what torch.autograd returns for
 * oracle/preprocess_oracle.py: a clamp passes the gradient at its bounds (0 and 1 inclusive); max and min over the
 * channels give it to the lowest channel index among ties; a select differentiates the selected branch only; floor, the
 * fraction of the hue, comparisons and the hue sector contribute nothing (so a white pixel with hue 0.2 and cotangent
 * (1, 2, 3) has gradient (6, 0, 0)).  A record's (cos_a, sin_a) must be a rotation (cos^2 + sin^2 = 1) and its order a
 * permutation or order[0] < 0, as the forward documents them.
 * No atomics: the contrast sum is per-block partials folded per image in a fixed order, the rotation's transpose is a
 * gather; d_src is always overwritten, every element, by one plain store; two calls on the same inputs give the same bits.
 * The caller's stream only, no allocation, no copy, no host synchronisation.
 * scratch: sgl_op_preprocess_aug_bwd_scratch_bytes() bytes of device memory, 4-byte aligned: the resize tables of
 * sgl_op_preprocess_bwd_scratch_bytes(), 2 B floats (the grey means, the contrast mean terms), B ceil(S^2 / 256) floats
 * (partials) and two fp32 (B,3,S,S) images (the gradients in front of and behind the rotation).  The size function
 * returns 0 for a dimension < 1.
 * Refused before anything is enqueued, d_src untouched: d_out, src, aug, d_src or scratch NULL SGL_ERR_NULL; std == 0 or
 * a dimension < 1 SGL_ERR_BAD_SHAPE; Hs > 16 * S or Ws > 16 * S SGL_ERR_UNSUPPORTED (the forward's limit); scratch_bytes
 * too small SGL_ERR_WORKSPACE. */
size_t sgl_op_preprocess_aug_bwd_scratch_bytes(int B, int Hs, int Ws, int S);
int sgl_op_preprocess_aug_bwd(const float* d_out, const void* src, int src_is_u8_nhwc, int B, int Hs, int Ws, int S,
                              float std, const sgl_aug_sample* aug, float* d_src, void* scratch, size_t scratch_bytes,
                              sgl_stream stream);

/* Video tail (hidf_video_classifier.py:304-316): per-frame embeddings f (B*T, D) fp32 -> each frame L2-normalised ->
 * mean over the T frames of a clip -> out (B, D); inv_norm (B*T) keeps 1/|f_t| for the backward
 * d f_t = (g - fhat_t (fhat_t . g)) / (T |f_t|), g = d out[b].
 * fwd: D <= 16380 (the clip's accumulator is D floats of LDS: D * 4 + 16 bytes within 64 KiB); a larger D is
 * SGL_ERR_BAD_SHAPE.  Squares are summed in fp32: inv_norm is accurate to (D / 512 + 12) * 2^-24 relative (the D-term
 * sum, sqrt and the division) as long as the squares are normal fp32 numbers, |f_t|^2 / D >= 2^-126 (|f_t| >= 1.1e-19 sqrt(D));
 * below that each square rounds by up to 2^-150 absolute and the relative error of inv_norm grows to
 * D * 2^-151 / |f_t|^2 (|f_t| = 1e-18: 4e-7 at D = 1152, 6e-6 at D = 16380).  A squared norm that overflows fp32
 * (|f_t| > 1.8e19) gives inv_norm 0, one that underflows to 0 gives inf. */
int sgl_op_l2norm_tmean_fwd(const float* f, float* out, float* inv_norm, int B, int T, int D, sgl_stream stream);
int sgl_op_l2norm_tmean_bwd(const float* f, const float* inv_norm, const float* dout, float* df, int B, int T, int D,
                            sgl_stream stream);

/* ---- SID mask-decoder tail, second half (Siglip2sidafrozen.py:731-745,174-181) -------------------
 * y = sigmoid(g) * x on n elements (the channel gate applied to the concatenated taps, `gate * x` at :741-742), and its
 * backward: dx = dy * sigmoid(g), dg = dy * x * s(1-s) (gradient w.r.t. the PRE-sigmoid gate; dg / dx may be NULL).
 * dtype f32 or bf16; n % 4 (f32) / n % 8 (bf16) == 0; 16-byte aligned pointers. */
int sgl_op_gate_mul(const void* g, const void* x, void* y, size_t n, int dtype, sgl_stream stream);
int sgl_op_gate_mul_bwd(const void* dy, const void* g, const void* x, void* dg, void* dx, size_t n, int dtype,
                        sgl_stream stream);
/* bce_dice_loss (:174-181) evaluated straight from the LOW-RESOLUTION logit map: logits_lr (B,g,g) fp32 is what the 1x1
 * head produces on the token grid; every one of the S*S output pixels is its bilinear (align_corners=False, as
 * F.interpolate at :743) interpolation, computed in registers, so the (B,1,S,S) logits never exist in HBM.
 * fwd: partial[b][chunk][4] = {sum bce, sum p*t, sum p, sum t} over 8 output rows (chunks = sgl_op_seg_loss_chunks(S));
 *      the caller folds the chunks (fixed order) and forms  bce_w * mean(bce) + dice_w * (1 - mean_b(2I/(P+T+eps))).
 * bwd: dlogits_lr[b] = transposed interpolation of  coef[b][0]*(p - t) + coef[b][1]*p(1-p)*(2tD - 2I)/D^2,
 *      sums[b] = the folded forward sums {.., I, P, T}, D = P + T + eps; gathered per low-res pixel, no atomics. */
int sgl_op_seg_loss_chunks(int S);
int sgl_op_seg_loss_fwd(const float* logits_lr, const float* targets, float* partial, int B, int g, int S,
                        sgl_stream stream);
int sgl_op_seg_loss_bwd(const float* logits_lr, const float* targets, const float* sums, const float* coef,
                        float* dlogits_lr, int B, int g, int S, float eps, sgl_stream stream);

/* combined_segmentation_loss (:69-172, the --use_enhanced_loss branch of the train step at :1379-1386) from the same
 * operands: BCE + focal + Dice + boundary-weighted BCE + IoU + the smoothness form of the morphological term (the branches
 * taken without Kornia).  z, p = sigmoid(z) and bce_px = max(z,0) - z t + log(1 + exp(-|z|)) of an output pixel are formed
 * exactly as by sgl_op_seg_loss_fwd.  n = images with a mask, N = n S^2.
 *   focal     alpha_t q^2 bce_px,  q = p + t - 2 p t,  alpha_t = alpha t + (1 - alpha)(1 - t)  (gamma = 2), mean over N
 *             d/dz = alpha_t (2 q (1 - 2t) p(1-p) bce_px + q^2 (p - t)) / N
 *   boundary  (1 + 3 beta) bce_px,  beta = [s > 0] - [s == 9],  s = fp32 sum of the nine zero-padded 3x3 neighbours of t in
 *             row-major order (dilate - erode, exact for {0,1} masks), mean over N;  d/dz = (1 + 3 beta)(p - t) / N
 *   iou       1 - I / U per image, U = sum p + sum t - I + smooth, I = sum p t, mean over n
 *             d/dz = -p(1-p) (t U - I (1 - t)) / (n U^2)
 *   morph     mean |p[x+1] - p[x]| + mean |p[y+1] - p[y]|, each over n S (S-1) pairs
 *             d/dz = p(1-p) (sum over the <= 4 neighbours of sign(p - p_nb)) / (n S (S-1)),  sign(0) = 0
 * terms: SGL_SEG_TERM_* bits selecting the three optional per-pixel computations.  Without a bit its sums are written as 0,
 *        its coefficient is not read as a term, and the work behind it (the 3x3 mask neighbourhood, the neighbour sigmoids)
 *        is not done.  BCE, Dice and IoU are always available.  Another bit -> SGL_ERR_UNSUPPORTED.
 * fwd: partial[b][chunk][8] = {sum bce_px, sum p t, sum p, sum t, sum focal, sum boundary, sum |dp/dx|, sum |dp/dy|} over 8
 *      output rows (chunks = sgl_op_seg_loss_chunks(S)); the vertical pair (i, i+1) belongs to the chunk of row i.
 * bwd: sums[b][8] = the chunks of image b folded by the caller in a fixed order (I, sum p, sum t are read);
 *      coef[b][6] = {c_bce, c_dice, c_focal, c_boundary, c_iou, c_tv} = upstream * weight * {1/N, -1/n, 1/N, 1/N, -1/n,
 *      1/(n S (S-1))}, all 0 for an image without a mask;
 *      dlogits_lr[b] = transposed interpolation of
 *        c_bce (p - t) + c_dice p(1-p)(2 t D - 2 I)/D^2 + c_focal alpha_t (2 q (1-2t) p(1-p) bce_px + q^2 (p - t))
 *        + c_boundary (1 + 3 beta)(p - t) + c_iou p(1-p)(t U - I (1-t))/U^2 + c_tv p(1-p) sum_nb sign(p - p_nb),
 *      D = sum p + sum t + eps; gathered per low-res pixel in a fixed order, no atomics, no scratch: bitwise reproducible.
 * Where both taps of an axis are the same logit (the clamped last rows / columns) the weight is taken as 0, so z there is
 * that logit itself rather than l (1 - w) + l w (at most an ulp apart).  Two output pixels whose taps and weights coincide
 * (all clamped border rows / columns, g = 1) therefore hold bit-equal p: their smoothness term and its gradient are exact
 * zeros, as in exact arithmetic.
 * Refused before anything is enqueued, nothing written: a NULL pointer -> SGL_ERR_NULL; B or g <= 0, S < 2 (the mean over
 * S - 1 pairs is undefined), g > 4096, S > 2048 (rows of p staged in LDS) -> SGL_ERR_BAD_SHAPE. */
#define SGL_SEG_TERM_FOCAL 1
#define SGL_SEG_TERM_BOUNDARY 2
#define SGL_SEG_TERM_TV 4
int sgl_op_seg_loss_ex_fwd(const float* logits_lr, const float* targets, float* partial, int B, int g, int S, int terms,
                           float alpha, sgl_stream stream);
int sgl_op_seg_loss_ex_bwd(const float* logits_lr, const float* targets, const float* sums, const float* coef,
                           float* dlogits_lr, int B, int g, int S, int terms, float alpha, float eps, float smooth,
                           sgl_stream stream);

/* The localisation metrics of the validation loop (:183-240 dice_iou_from_logits / sweep_mask_thresholds, :1078-1106
 * PixelAUCBuffer) as integer counts, again straight from the low-resolution logit map, in one pass and without a host
 * synchronisation.  Per output pixel of every selected image:
 *   z = the bilinear (align_corners=False) value of its four low-res logits, formed exactly as in sgl_op_seg_loss_fwd (the
 *       loss and the metrics see the same fp32 logit);
 *   c = 1 when its target is > 0.5, else 0 (SID masks are {0,1}, :908,913; a SOFT mask is thresholded at 0.5);
 *   k = the number of cuts strictly below z, so  z > cuts[j]  <=>  j < k  (a NaN logit is below every cut: k = 0);
 *   hist[b][c][k] += 1;
 *   auc_hist[c][min(max(floor((z + 16) * NB / 32), 0), NB - 1)] += 1  with NB = SGL_SEG_EVAL_AUC_BINS: uniform bins of
 *       width 1/128 on logits in [-16, 16), everything outside in the end bins, NaN in bin 0.
 * logits_lr [B][g][g] fp32; targets [B][S][S] contiguous, target_dtype SGL_DTYPE_F32 or SGL_DTYPE_U8 (any element-aligned
 * address: 16-byte loads start at the first 16-byte boundary of each 64-row band); sel [B] bytes, NULL = every image;
 * cuts [K] fp32 in DEVICE memory, strictly increasing (the caller's contract: not checked here), 1 <= K <= 64.
 * hist [B][2][K+1] int32 is OVERWRITTEN (an image with sel[b] == 0 gets an all-zero row); auc_hist [2][NB] unsigned 64-bit
 * is ACCUMULATED into (zero it once per evaluation; images with sel[b] == 0 add nothing) and may be NULL, which skips it.
 * All counters are integers added with atomics: the result does not depend on the order and is bitwise reproducible.
 * Refused before anything is enqueued: logits_lr, targets, cuts or hist NULL -> SGL_ERR_NULL; B, g or S <= 0, K < 1,
 * K > 64, S > 32768, g > 32768, fp32 targets not 4-byte aligned -> SGL_ERR_BAD_SHAPE; another target_dtype ->
 * SGL_ERR_UNSUPPORTED. */
#define SGL_SEG_EVAL_AUC_BINS 4096
int sgl_op_seg_eval_auc_bins(void);   /* SGL_SEG_EVAL_AUC_BINS, for callers that bind the library without the header */
int sgl_op_seg_eval(const float* logits_lr, const void* targets, int target_dtype, const uint8_t* sel, const float* cuts,
                    int K, int32_t* hist, unsigned long long* auc_hist, int B, int g, int S, sgl_stream stream);

/* ---- optimizer step tail -----------------------------------------------------------------
 * Replaces, for a list of fp32 tensors, the reference's per-step pair
 *     torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)   Siglip2sidafrozen.py:1396
 *     torch.optim.AdamW(...).step()                                  Siglip2sidafrozen.py:1241-1244,1398
 * without a host synchronisation: the clip coefficient stays in device memory.
 * One table entry per parameter tensor; the table, the block map and the scratch live in DEVICE memory owned by the
 * caller.  g == NULL marks a parameter without a gradient this step (skipped, as torch does). */
typedef struct {
  float* p;        /* fp32 parameter, updated in place */
  const float* g;  /* fp32 gradient (not modified: the clip coefficient is applied on the fly) */
  float* m;        /* exp_avg */
  float* v;        /* exp_avg_sq */
  uint64_t n;      /* elements */
  float lr, weight_decay; /* of the parameter group the tensor belongs to */
} sgl_adamw_tensor;
/* HOST helper: cuts tensor t into ceil(numel[t]/4096) chunks and writes (tensor, chunk) int32 pairs into blockmap
 * (host memory, capacity in pairs; may be NULL to size it).  Returns the number of pairs (= workgroups). */
int64_t sgl_adamw_plan(const uint64_t* numel, int ntensors, int32_t* blockmap, int64_t capacity_pairs);
/* norm_and_coef[0] = sqrt(sum g^2) over the table; [1] = min(1, max_norm/(norm+1e-6)) (1 when max_norm <= 0).
 * partials: nblocks floats of scratch.  Reduction order is fixed: bitwise reproducible. */
int sgl_op_grad_norm(const sgl_adamw_tensor* table, const int32_t* blockmap, int64_t nblocks, float max_norm,
                     float* partials, float* norm_and_coef, sgl_stream stream);
/* One AdamW step (decoupled weight decay, torch/optim/adamw.py operation order) on every tensor of the table;
 * step >= 1 is the bias-correction exponent; norm_and_coef (may be NULL) is the output of sgl_op_grad_norm. */
int sgl_op_adamw(const sgl_adamw_tensor* table, const int32_t* blockmap, int64_t nblocks, double beta1, double beta2,
                 double eps, int step, const float* norm_and_coef, sgl_stream stream);
/* ---- AdamW that also leaves behind everything a parameter update invalidates (kernel work-list k11) -----------------
 * Per table entry, optional destinations written in the same pass as the update:
 *   dst / dst_t : compute-dtype (dtype) row-major copy dst[(r-row0)*ld + c] and transposed copy dst_t[c*ld_t + (r-row0)]
 *                 of the rows r >= row0 of the [rows, cols] parameter: the encoder's weight shadows (sgl_prepare_weights
 *                 layouts; pad regions are never touched), so no re-cast is needed before the next forward;
 *   dst_f32     : fp32 copy of a 1-D tensor (the fused qkv / fc1 bias vectors of the shadow arena);
 *   ema         : ExponentialMovingAverage shadow (cifake_binary_classifier.py:222-225): ema = ema*decay + p*(1-decay);
 *   group       : index into the per-launch (lr, weight_decay) list (changing the learning rate every step then needs no
 *                 table upload); -1 = use the table entry's own lr / weight_decay.
 * Entries with dst or dst_t are walked in 64x64 tiles: plan them as ceil(rows/64)*ceil(cols/64) chunks, i.e. pass
 * that count * 4096 as the tensor's numel to sgl_adamw_plan. */
typedef struct {
  void* dst;
  void* dst_t;
  float* dst_f32;
  float* ema;
  int ld, ld_t, rows, cols, row0, dtype, group, reserved;
} sgl_adamw_aux;
/* HOST helper: fills aux[i].{dst, dst_t, dst_f32, ld, ld_t, rows, cols, row0, dtype} for every table entry whose .p is one
 * of the master tensors in `w` that has a copy in the shadow arena `shadow` of `ctx` (table and aux are HOST arrays of
 * ntensors entries; other aux fields are left untouched).  Returns the number of entries bound. */
int sgl_adamw_bind_shadows(const sgl_ctx* ctx, const sgl_weights* w, void* shadow, const sgl_adamw_tensor* table_host,
                           sgl_adamw_aux* aux_host, int ntensors);
/* sgl_op_grad_norm with a gradient scale s (gradients are rank sums, s = 1/world): [0] = s*norm,
 * [1] = s*min(1, max_norm/(s*norm + 1e-6)) (= s when max_norm <= 0). */
int sgl_op_grad_norm_scaled(const sgl_adamw_tensor* table, const int32_t* blockmap, int64_t nblocks, float max_norm,
                            float grad_scale, float* partials, float* norm_and_coef, sgl_stream stream);
/* group_lr_wd_host: HOST array of ngroups (<= 16) {lr, weight_decay} pairs passed by value with the launch, or NULL with
 * ngroups = 0; ema_decay is used by entries with aux.ema != NULL. */
int sgl_op_adamw_ex(const sgl_adamw_tensor* table, const sgl_adamw_aux* aux, const int32_t* blockmap, int64_t nblocks,
                    double beta1, double beta2, double eps, int step, const float* norm_and_coef,
                    const float* group_lr_wd_host, int ngroups, double ema_decay, sgl_stream stream);
/* ---- the same step tail under torch.amp.GradScaler (scaler.scale(loss).backward(); scaler.step(opt); scaler.update(),
 * Siglip2sidafrozen.py:1276,1390-1397, cifake_binary_classifier.py:831-841, hidf_video_classifier.py:388-402) ------
 * The gradients in the table are loss-scaled; the scale and the scaler's inf flag are DEVICE values, and so is the
 * decision to skip the step: no unscale pass, no host synchronisation.  Caller-owned device state, 32 bytes, 4-byte
 * aligned, zero it once (hipMemset) before the first call: */
typedef struct {
  float found_inf;      /* 1.0f when this step is skipped, else 0.0f; written by sgl_op_grad_norm_amp (a float, so that it
                           can be handed to GradScaler.update() as the found-inf tensor it sums) */
  int32_t skipped;      /* running count of skipped steps */
  float inv_bc1;        /* 1 / (1 - beta1^t)       of the last sgl_op_adamw_amp launch, t = step - skipped */
  float inv_sqrt_bc2;   /* 1 / sqrt(1 - beta2^t) */
  int32_t reserved[4];
} sgl_amp_state;
/* sgl_op_grad_norm_scaled for loss-scaled gradients.  amp_scale[0] is the loss scale (NULL = 1), found_inf_in[0] != 0
 * says the caller already found an inf / NaN (NULL = 0); both are device pointers.  Every gradient is multiplied by
 * inv = 1/amp_scale[0] BEFORE it is squared (a finite scaled gradient then never overflows in its square; exact for the
 * power-of-two scales GradScaler produces); block and final summation order are sgl_op_grad_norm's.  Writes
 *   norm_and_coef[0] = world_scale * ||g/scale||                             the TRUE norm
 *   norm_and_coef[1] = (min(1, max_norm/([0] + 1e-6)) * world_scale) * inv   (max_norm <= 0: (world_scale) * inv), so that
 *                      for a power-of-two scale g_scaled*[1] has the bits g_true*[1] has in sgl_op_grad_norm_scaled
 *   state->found_inf = 1 when found_inf_in[0] != 0 or the sum of squares is not finite, else 0; when 1, also
 *                      state->skipped += 1.
 * A not-finite sum is an inf or NaN gradient, or a true norm beyond fp32's range (the block sums are fp32, so from about
 * 1.8e19 up), where torch's own clip coefficient would already be 0 or NaN: such a step is skipped too.
 * nblocks == 0 is allowed (the sum is 0: only found_inf_in decides).  Refused before anything is enqueued: table,
 * blockmap, partials, norm_and_coef or state NULL -> SGL_ERR_NULL; nblocks < 0 or > 2^31-1, or amp_scale, found_inf_in or
 * state not 4-byte aligned -> SGL_ERR_BAD_SHAPE. */
int sgl_op_grad_norm_amp(const sgl_adamw_tensor* table, const int32_t* blockmap, int64_t nblocks, float max_norm,
                         float world_scale, const float* amp_scale, const float* found_inf_in, float* partials,
                         float* norm_and_coef, sgl_amp_state* state, sgl_stream stream);
/* sgl_op_adamw_ex that obeys `state`: with state->found_inf == 1 every block returns before its first store (parameters,
 * exp_avg, exp_avg_sq, dst / dst_t, dst_f32 and ema keep their bits).  The host cannot know how many steps were skipped
 * without a synchronisation, so `step` >= 1 counts CALLS; the effective step is t = max(1, step - state->skipped), and
 * its bias corrections are formed on the device in double and rounded to float (the host formulas of sgl_op_adamw_ex)
 * by a one-thread launch in front of the update, which leaves them in state->inv_bc1 / inv_sqrt_bc2.
 * Refused before anything is enqueued: table, aux, blockmap or state NULL, or group_lr_wd_host NULL with ngroups > 0
 * -> SGL_ERR_NULL; nblocks < 0 or > 2^31-1, step < 1, ngroups outside [0, 16], state not 4-byte aligned ->
 * SGL_ERR_BAD_SHAPE. */
int sgl_op_adamw_amp(const sgl_adamw_tensor* table, const sgl_adamw_aux* aux, const int32_t* blockmap, int64_t nblocks,
                     double beta1, double beta2, double eps, int step, const float* norm_and_coef,
                     const float* group_lr_wd_host, int ngroups, double ema_decay, sgl_amp_state* state,
                     sgl_stream stream);
/* Weight EMA of the CiFake trainer (ExponentialMovingAverage.update,cifake_binary_classifier.py:222-225):
 * shadow = shadow*decay + p*(1-decay) for every table entry, with p = entry.p (read only) and shadow = entry.m. */
int sgl_op_ema(const sgl_adamw_tensor* table, const int32_t* blockmap, int64_t nblocks, double decay,
               sgl_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGLIP_HIP_H */
