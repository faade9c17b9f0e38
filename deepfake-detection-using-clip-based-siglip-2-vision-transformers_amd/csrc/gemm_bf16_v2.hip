// bf16 / fp16 MFMA GEMMs for gfx950, K-step 64, 512 threads = 8 waves, operands streamed global -> LDS by LDS-DMA
// (buffer_load_dwordx4 ... lds, 1 KiB per wave instruction, no VGPR staging), two LDS stages.  Two kernels:
//   gemm_nt6_kernel<Tile, ...>   NT on a tile geometry: NtTile256 (256 x 256), NtTile384 (384 x 192) or NtTile288 (256 x 288,
//                                the QKV scatter of 72-wide heads only), see the structs
//   gemm_tn6_kernel<Tile, ...>   TN on the first two geometries
// Both main loops run anti-phase wave groups, four barrier-separated slots per K-step (see the comments above them),
// and share the LDS images, the tile order and one staged epilogue (store_tile_pp; store_tile_qkv_heads where a tile is
// whole heads).  gemm_nt_bf16 / gemm_tn_bf16 (gemm_bf16.hip) send the shapes that fill the chip here, through gemm_nt256 /
// gemm_nt384 / gemm_nt288 / gemm_tn256 / gemm_tn384 at the end of this file, and hold the rules that choose the tile (and,
// for TN, the split).
//
//   nt : C[M,N]   = A[M,K] · B[N,K]ᵀ           (forward projections, dX with transposed weight shadows)
//   tn : C[N1,N2] (+)= Σ_m A[m,N1] · B[m,N2]    (dW; token index is the MFMA k index via ds_read_b64_tr_b16)
//
// Arithmetic intensity of both tiles: 2*256*256*64 / (2*256*64*2 B) = 2*384*192*64 / ((384+192)*64*2 B) = 128 FLOP per
// LDS-staged byte (the 128x128 tile of gemm_bf16.hip has 64 and is L2->LDS bandwidth bound near 0.6-0.7 PFLOP/s on this chip).
//
// LDS-DMA writes lane-linear (wave-uniform base + lane*16), so the bank-conflict swizzles are applied to each
// lane's SOURCE address and again on the fragment reads (same involution on both sides):
//   NT image [rows][64 k]       128-B rows: slot s of row r holds source chunk s ^ (r & 7)
//   TN image [64 m][BM or BN n] 512-, 768- or 384-B rows: slot s of row m holds source chunk s ^ tn_swz(m), see gemm_tn6_kernel
// blockIdx -> tile is XCD-aware (unit_of_block / tile_of_unit below): each XCD works through a contiguous chunk of
// a grouped tile order, so its concurrent workgroups share A and B panels in its private L2.  Measured with
// rocprofv3 FETCH_SIZE on the fc1 shape: the earlier "row panel per XCD" map fetched 6x the algorithmic bytes
// because the 10 MB weight panel thrashed every 4 MiB L2.  Placement affects speed only.
#include <stdlib.h>
#ifdef SGL_TIMELINE
#include <stdio.h>
#include <string.h>
#endif

#include "common.hip.h"
#include "epilogue.hip.h"
#include "kernels.h"

namespace sgl {

constexpr int T_BK = 64;

// ------------------------------------------------------------------------------------------------------
// Tile geometries.  A geometry states the tile, the MI x MJ accumulator blocks (16 x 16) of a wave, the wave map and
// which 8-row pieces of the B image a wave's DMA instructions move; everything else follows here, once.
// ------------------------------------------------------------------------------------------------------
template <int BM_, int BN_, int MI_, int MJ_, bool SPLIT_B_ = false, int CT_LD_ = BN_ + 4, int QKV_HD_ = 0, int QKV_HDP_ = 0>
struct NtTileShape {
  static constexpr int BM = BM_, BN = BN_, MI = MI_, MJ = MJ_;
  static constexpr int WM = 16 * MI, WN = 16 * MJ;     // wave tile
  static constexpr int NWR = BM / WM, NWC = BN / WN;   // wave grid
  static constexpr int BNI = (BN + 63) / 64 * 64;      // rows of the B image: DMA pieces are dealt in whole 64-row rounds, rows
                                                       // past BN are requested out of range (zeros) and never read
  static constexpr int OPA = BM * T_BK * 2;            // bytes of A per stage; the B image follows it
  static constexpr int STAGE = (BM + BNI) * T_BK * 2;
  static constexpr int LDS = 2 * STAGE;
  // Which operand the main loop reads in halves (see the schedule above gemm_nt6_kernel).  SPLIT_B = false: A by row
  // blocks (units A0, B, A1); true: B by column blocks (units A, B0, B1; B0 = the first J0 column blocks of every wave
  // column, B1 = the other J1).  The choice balances the fragment reads of the two read slots.
  static constexpr bool SPLIT_B = SPLIT_B_;
  static constexpr int J0 = (MJ + 1) / 2, J1 = MJ - J0;
  // DMA instructions (8 image rows = 1 KiB each) per wave and unit, in stream order; NI per K-step is also the vmcnt
  // immediate of the read slots.  The pad rows of the B image ride with B0, which makes its pieces a multiple of 8.
  static constexpr int P0 = SPLIT_B ? BM / 64 : BM / 128;
  static constexpr int P1 = SPLIT_B ? (NWC * J0 * 16 + BNI - BN) / 64 : BNI / 64;
  static constexpr int P2 = SPLIT_B ? (NWC * J1 * 16) / 64 : BM / 128;
  static constexpr int NI = P0 + P1 + P2;
  static constexpr int CT_LD = CT_LD_;                 // fp32 epilogue staging stride (default: 4 mod 64 banks)
  // EPI_QKV with whole heads per tile (BN % QKV_HD == 0): the head-major epilogue walk (store_tile_qkv_heads) for heads
  // of QKV_HD columns stored QKV_HDP wide; 0 = the row-major walk of store_tile_pp
  static constexpr int QKV_HD = QKV_HD_, QKV_HDP = QKV_HDP_;
  static_assert(NWR * WM == BM && NWC * WN == BN && NWR * NWC == 8, "8 waves = 512 threads cover the tile");
  static_assert(BM % 128 == 0 && 64 % NWR == 0 && (64 / NWR) % 16 == 0, "pieces, passes");
  static_assert(SPLIT_B ? ((NWC * J0 * 16 + BNI - BN) % 64 == 0 && (NWC * J1 * 16) % 64 == 0 && (J0 * 16) % 8 == 0)
                        : (MI % 2 == 0 && BN % 64 == 0), "every wave issues the same number of pieces of every unit");
  static_assert(QKV_HD == 0 || (BN % QKV_HD == 0 && QKV_HD % 8 == 0 && QKV_HDP % 8 == 0 && QKV_HDP >= QKV_HD &&
                                (64 * (BN / QKV_HD) * (QKV_HDP / 8)) % 512 == 0), "whole heads, whole chunk rounds");
  static_assert(CT_LD >= BN && CT_LD % 4 == 0, "16-byte aligned staging rows");
  static_assert(LDS <= 160 * 1024 && 64 * CT_LD * 4 <= LDS, "two stages, and the epilogue image, in 160 KiB of LDS");
};

// 256 x 256 (2 x 64 KiB): waves 2 (rows) x 4 (columns), 128 x 64 each.  The two waves sharing a SIMD (w, w+4) sit in
// different column halves.  In a half-empty last column tile (0 < N % 256 <= 128) the waves of the empty half skip their
// instructions (`active`) but still take part in every barrier, so the workgroup holds its CU for the whole K loop:
// that tile takes as long as a full one (the skipped work saves power, not time).  That is why N = 1152 = 4.5 tiles has
// the other geometry.
struct NtTile256 : NtTileShape<256, 256, 8, 4> {
  static __device__ __forceinline__ int wr(int w) { return (w >> 1) & 1; }
  static __device__ __forceinline__ int wc(int w) { return (w & 1) + 2 * (w >> 2); }
  // B piece q (of P1 = 4) of wave w: q < 2 is "BX", the first 32 columns of every wave column, q >= 2 "BY", the other 32
  static __device__ __forceinline__ int b_row(int w, int q) {
    const int ul = 16 * w + 8 * (q & 1);
    return (ul >> 5) * 64 + (ul & 31) + 32 * (q >> 1);
  }
  static constexpr bool takes(int epi) { return true; }
};

// 384 x 192 (2 x 72 KiB): waves 4 (rows) x 2 (columns), 96 x 96 each (0.33 fragment reads per MFMA against 0.375), the
// two waves of a SIMD again in different column halves.  For outputs 1152 = 6 x 192 wide there is no half-empty column
// tile, and at the bench batch 93,312 = 243 x 384 rows give 1,458 tiles of 1.125 x the work where NtTile256 runs 1,825.
// N need not divide by 192 for correctness.  EPI_STORE and EPI_RES_F32 (NT), EPI_F32 (the TN kernel's slabs and atomics)
// only: nothing else is sent here.
struct NtTile384 : NtTileShape<384, 192, 6, 6> {
  static __device__ __forceinline__ int wr(int w) { return w & 3; }
  static __device__ __forceinline__ int wc(int w) { return w >> 2; }
  static __device__ __forceinline__ int b_row(int w, int q) { return 8 * (3 * w + q); }
  static constexpr bool takes(int epi) { return epi == EPI_STORE || epi == EPI_RES_F32 || epi == EPI_F32; }
};

// 256 x 288 (2 x 72 KiB): waves 4 (rows) x 2 (columns), 64 x 144 each, the two waves of a SIMD in different column
// halves.  288 = 4 x 72: for the QKV projection of a model with 72-wide heads (N = 3 heads 72, heads % 4 == 0) a tile
// holds heads 4 tile_n .. 4 tile_n + 3 from its column 0, N = 3456 is 12 whole tiles where NtTile256 runs 13.5 (14), and
// the epilogue writes every head's rows as one run of 160-byte rows (store_tile_qkv_heads).  B is the operand read in
// halves: all of A plus column blocks 0-4 make 18 fragment reads in R1, column blocks 5-8 make 8 in R2 (A in halves
// would be 22 + 4).  The B image has 320 rows; rows 288..319 are the four pad pieces of unit B0 (24 pieces = 3 per wave),
// always out of range.  CT_LD = 336: with it the 32-byte chunk reads of the head-major walk (two ds_read_b128 per lane,
// halves swapped on lane bit 3) touch every bank once per 16-lane group in all 5 x 8 wave reads of a pass; the staging
// stores are 2-way with it (4 rows = 0 mod 32 banks), which a ds_write_b32 hides behind its register transfer, and no
// stride has both (profiles/nt288_resources.txt).  EPI_QKV with 16-bit outputs only; gemm_nt_mfma checks head_dim, head_dim_pad and N before it sends a launch here.
struct NtTile288 : NtTileShape<256, 288, 4, 9, true, 336, 72, 80> {
  static __device__ __forceinline__ int wr(int w) { return w & 3; }
  static __device__ __forceinline__ int wc(int w) { return w >> 2; }
  // B piece q of wave w in unit B0 (half 0, P1 = 3 per wave) / B1 (half 1, P2 = 2 per wave)
  static __device__ __forceinline__ int b_row(int w, int half, int q) {
    if (half == 0) {
      const int piece = P1 * w + q;   // 0..19: 2 J0 = 10 pieces of each wave column; 20..23: the pad rows
      return piece < NWC * 2 * J0 ? WN * (piece / (2 * J0)) + 8 * (piece % (2 * J0)) : BN + 8 * (piece - NWC * 2 * J0);
    }
    const int piece = P2 * w + q;     // 0..15: 2 J1 = 8 pieces of each wave column
    return WN * (piece / (2 * J1)) + 16 * J0 + 8 * (piece % (2 * J1));
  }
  static constexpr bool takes(int epi) { return epi == EPI_QKV; }
};

constexpr int gcd_of(int a, int b) { return b == 0 ? a : gcd_of(b, a % b); }

// accumulators -> LDS (64 tile rows per pass) -> row-contiguous 16-byte chunks -> fused epilogue.
// A pass stages 64 / NWR rows of every wave row (BLK of each wave's MI sixteen-row blocks) in a [64][CT_LD] fp32 image:
// LDS stores then come from both SIMD halves at once (stores issued from SIMDs {0,1} only, as a "rows of wr == 0 first"
// order would, run at half rate: MI355X_MICROARCH.md, LDS section).  The workgroup then walks the image's chunks in
// row-major order, chunk t + 512 q for thread t, so a wave store covers whole output rows.  The column of a thread's
// chunk repeats in q with period P = lcm(CPR, 512) / 512 (CPR chunks per row: 1 on the 256-wide tile, 3 on the 192-wide
// one), so everything that depends only on the column (bias, range check, the QKV decomposition) exists P times per
// thread and is loaded / decomposed ONCE.  The per-chunk operands that come from memory (the fp32 residual, the saved
// pre-activation of GELU') are requested one pass ahead of their use, BEFORE the stores of the pass in between: vmcnt
// retires in order, so a load issued behind a store cannot be waited for without waiting for that store's
// acknowledgement first — with the loads inside the chunk loop (epi_apply) every chunk paid an HBM write round trip
// (residual epilogue: 60 k cycles per tile against 25 k with this order; out_proj GEMM 410 -> 330 us at B = 128).
// The caller has drained its DMA (vmcnt(0)), so every barrier here orders LDS traffic only (lds_barrier): the global
// stores stay in flight across passes.
template <typename G, int EPI, typename TOut>
__device__ __forceinline__ void store_tile_pp(char* smem, f32x4 (&acc)[G::MI][G::MJ], int wr, int wc, int lane, int t,
                                              int m0, int n0, int M, int N, const EpiParams& p) {
  static_assert(G::takes(EPI), "this tile geometry is not dispatched with this epilogue");
  float* ct = reinterpret_cast<float*>(smem);
  const int g = lane >> 4, c16 = lane & 15;
  constexpr int NV = (sizeof(TOut) == 4) ? 4 : 8;
  constexpr int CT_LD = G::CT_LD;
  constexpr int CPR = G::BN / NV;                       // chunks per row
  constexpr int WR_ROWS = 64 / G::NWR;                  // rows a wave row contributes per pass
  constexpr int BLK = WR_ROWS / 16;                     // 16-row blocks of every wave per pass
  constexpr int NPASS = G::BM / 64;
  constexpr int QN = (64 * CPR) / 512;                  // chunks per thread and pass
  constexpr int P = CPR / gcd_of(CPR, 512);             // column period of the chunk walk
  static_assert(NPASS * BLK == G::MI && (64 * CPR) % 512 == 0 && (512 * P) % CPR == 0, "staging image and chunk walk");
  // staging row `row` of pass `pass` holds this tile row
  auto grow_of = [&](int pass, int row) { return m0 + (row / WR_ROWS) * G::WM + pass * WR_ROWS + row % WR_ROWS; };
  constexpr bool HAS_BIAS = (EPI == EPI_BIAS_GELU || EPI == EPI_RES_F32 || EPI == EPI_QKV);
  int tcol[P], gcol[P];
  bool col_ok[P];
  float bias[P][NV];
  // QKV scatter: column -> (which, head, d) is fixed per column; element offset of row (b, n) is qkv_c0 + (b*H*T + n) * pad
  size_t qkv_c0[P];
  int qkv_pad[P];                                       // pad chunks behind the head's last data chunk
#pragma unroll
  for (int h = 0; h < P; ++h) {
    tcol[h] = ((t + 512 * h) % CPR) * NV;
    gcol[h] = n0 + tcol[h];
    col_ok[h] = gcol[h] < N;
#pragma unroll
    for (int j = 0; j < NV; ++j) bias[h][j] = 0.f;
    if constexpr (HAS_BIAS) {
      if (col_ok[h]) Vec<float, NV>::ld(p.bias + gcol[h], bias[h]);
    }
    qkv_c0[h] = 0;
    qkv_pad[h] = 0;
    if constexpr (EPI == EPI_QKV) {
      const int dm = p.heads * p.head_dim;
      const int which = gcol[h] / dm;
      const int hc = gcol[h] - which * dm;
      const int hd = hc / p.head_dim;
      const int d = hc - hd * p.head_dim;
      qkv_c0[h] = ((size_t)which * p.batch * p.heads + hd) * (size_t)p.tokens * p.head_dim_pad + d;
      qkv_pad[h] = (d + NV == p.head_dim) ? (p.head_dim_pad - p.head_dim) / NV : 0;
    }
  }
  float csum[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) csum[j] = 0.f;
  using PreT = u32x4;                       // one raw 16-byte chunk: 4 fp32 residuals / 8 bf16 (fp16) pre-activations
  constexpr bool HAS_PRE = (EPI == EPI_RES_F32 || EPI == EPI_GELU_BWD);
  PreT pre[2][QN];
  auto load_pre = [&](int pass, PreT (&dst)[QN]) {
    if constexpr (HAS_PRE) {
#pragma unroll
      for (int q = 0; q < QN; ++q) {
        const int h = q % P;
        const int grow = grow_of(pass, (t + 512 * q) / CPR);
        const void* src = (EPI == EPI_RES_F32)
                              ? (const void*)(p.res + (size_t)grow * p.ldr + gcol[h])
                              : (const void*)(reinterpret_cast<const TOut*>(p.aux) + (size_t)grow * p.ldaux + gcol[h]);
        dst[q] = (grow < M && col_ok[h]) ? *reinterpret_cast<const PreT*>(src) : PreT{0u, 0u, 0u, 0u};
      }
    }
  };
  load_pre(0, pre[0]);
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    if (pass + 1 < NPASS) load_pre(pass + 1, pre[(pass + 1) & 1]);
    lds_barrier();   // pass 0: every wave is done with the operand stages; later: the previous pass's chunk reads are done
#pragma unroll
    for (int i2 = 0; i2 < BLK; ++i2)
#pragma unroll
      for (int j = 0; j < G::MJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          ct[(wr * WR_ROWS + i2 * 16 + g * 4 + r) * CT_LD + wc * G::WN + j * 16 + c16] = acc[BLK * pass + i2][j][r];
    lds_barrier();
    if constexpr (EPI == EPI_F32) {
      if (p.atomic) {   // split-K: fp32 atomics shaped as 256 contiguous bytes per wave instruction (one dword per lane)
        float* outp = reinterpret_cast<float*>(p.out);
        const int w = t >> 6;
#pragma unroll 2
        for (int rr = 0; rr < 8; ++rr) {
          const int row = w + rr * 8;
          const int grow = grow_of(pass, row);
          if (grow >= M) continue;
#pragma unroll
          for (int h = 0; h < G::BN / 64; ++h) {
            const int col = lane + 64 * h;
            if (n0 + col < N) atomicAdd(outp + (size_t)grow * p.ldo + n0 + col, ct[row * CT_LD + col] * p.alpha);
          }
        }
        continue;
      }
    }
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      const int h = q % P;
      const int row = (t + 512 * q) / CPR;
      const int grow = grow_of(pass, row);
      if (grow < M && col_ok[h]) {
        float v[NV];
        Vec<float, NV>::ld(ct + row * CT_LD + tcol[h], v);
        if constexpr (EPI == EPI_RES_F32) {
          const f32x4 r = __builtin_bit_cast(f32x4, pre[pass & 1][q]);
          float rf[NV];
#pragma unroll
          for (int j = 0; j < NV; ++j) rf[j] = r[j];
          epi_res_f32<NV>(v, bias[h], rf, reinterpret_cast<float*>(p.out) + (size_t)grow * p.ldo + gcol[h]);
        } else if constexpr (EPI == EPI_BIAS_GELU) {
          epi_bias_gelu<TOut, NV>(p, v, bias[h], reinterpret_cast<TOut*>(p.out) + (size_t)grow * p.ldo + gcol[h],
                                  reinterpret_cast<TOut*>(p.out2) + (size_t)grow * p.ldo2 + gcol[h]);
        } else if constexpr (EPI == EPI_QKV) {
          // (Round 3 tried dealing a pass's chunks out head by head so that a wave store covers 6.4 whole 160-byte rows of
          // one head, 1 KiB contiguous instead of eight 144-byte pieces: QKV GEMM 853 -> 886 us, the per-chunk decode costs
          // more than the store pattern saves.  Not kept on this walk: head boundaries fall differently in every 256-wide
          // tile.  Where the tile is a whole number of heads the decode is three divisions by constants and the deal pays:
          // store_tile_qkv_heads below, which NtTile288 takes instead of this branch.)
          int b, n;
          qkv_split_row(grow, p.tokens, b, n);
          epi_qkv<TOut, NV>(v, bias[h],
                            reinterpret_cast<TOut*>(p.out) + qkv_c0[h] + ((size_t)b * p.heads * p.tokens + n) * p.head_dim_pad,
                            qkv_pad[h]);
        } else if constexpr (EPI == EPI_GELU_BWD) {
          float u[NV];
          if constexpr (NV == 8) {
            const lo_x8<TOut> ub = __builtin_bit_cast(lo_x8<TOut>, pre[pass & 1][q]);
#pragma unroll
            for (int j = 0; j < NV; ++j) u[j] = (float)ub[j];
          } else {
            const f32x4 uf = __builtin_bit_cast(f32x4, pre[pass & 1][q]);
#pragma unroll
            for (int j = 0; j < NV; ++j) u[j] = uf[j];
          }
          epi_gelu_bwd<TOut, NV>(p, v, u, reinterpret_cast<TOut*>(p.out) + (size_t)grow * p.ldo + gcol[h]);
#pragma unroll
          for (int j = 0; j < NV; ++j) csum[j] += v[j];
        } else {
          epi_apply<EPI, TOut, NV>(p, grow, gcol[h], N, v);
        }
      }
    }
  }
  if constexpr (EPI == EPI_GELU_BWD) {
    static_assert(P == 1, "the bias-gradient fold needs one column set per thread");
    epi_colsum_fold<512, G::BN, NV>(ct, csum, t, m0, n0, N, p);
  }
}

// EPI_QKV on a geometry whose tile is a whole number of heads (G::QKV_HD columns each, stored G::QKV_HDP wide): the staging
// of store_tile_pp, then a HEAD-major chunk walk.  The tile holds heads HPT tile_n .. HPT tile_n + HPT - 1 from column 0,
// and inside one image consecutive rows of a head are consecutive 2 QKV_HDP-byte rows of its [tokens][QKV_HDP] matrix, so
// chunk i = t + 512 q of a pass is
//     head = i / (64 CPH),  staging row = i % (64 CPH) / CPH,  c = i % CPH      (CPH = QKV_HDP / 8, constants all)
// and consecutive lanes store consecutive 16-byte chunks: a wave store is 1 KiB of consecutive bytes except where it
// crosses one of the pass's 16-row runs (the staging keeps every wave row's rows together) or an image boundary.  Chunks
// c >= QKV_HD / 8 are the pad columns and leave as +0 with the rest (they read the head's last data chunk again, a
// broadcast).  The bias is added on the accumulator side, MJ values per lane loaded before the first pass: a load issued
// behind the stores would wait for their acknowledgement (see above).  Same arithmetic as epi_qkv: (acc + bias) rounded
// to nearest.  A lane reads its 32 bytes as two ds_read_b128, columns 4..7 first on lanes with bit 3 set: with
// G::CT_LD that order covers the 64 banks exactly once per 16-lane group.
// The caller guarantees 16-bit outputs, N % G::BN == 0 and heads % HPT == 0 (a tile never straddles q / k / v).
template <typename G, typename TOut>
__device__ __forceinline__ void store_tile_qkv_heads(char* smem, f32x4 (&acc)[G::MI][G::MJ], int wr, int wc, int lane,
                                                     int t, int m0, int n0, int M, const EpiParams& p) {
  static_assert(G::takes(EPI_QKV) && G::QKV_HD > 0, "this tile geometry does not hold whole heads");
  float* ct = reinterpret_cast<float*>(smem);
  const int g = lane >> 4, c16 = lane & 15;
  constexpr int NV = 8, CT_LD = G::CT_LD;
  constexpr int HPT = G::BN / G::QKV_HD;                // heads per tile
  constexpr int CPH = G::QKV_HDP / NV;                  // chunks per head row, pad chunks included
  constexpr int DCH = G::QKV_HD / NV;                   // data chunks per head row
  constexpr int CHD = 64 * CPH;                         // chunks per head and pass
  constexpr int QN = (HPT * CHD) / 512;                 // chunks per thread and pass
  constexpr int WR_ROWS = 64 / G::NWR, BLK = WR_ROWS / 16, NPASS = G::BM / 64;
  static_assert(NPASS * BLK == G::MI, "staging image");
  float bias[G::MJ];
#pragma unroll
  for (int j = 0; j < G::MJ; ++j) bias[j] = p.bias[n0 + wc * G::WN + j * 16 + c16];
  // rows of [tokens][QKV_HDP] in front of (q|k|v, image 0, first head of the tile); head h of the tile is h * tokens further
  const int gh0 = n0 / G::QKV_HD, which = gh0 / p.heads;
  const int rows0 = (which * p.batch * p.heads + (gh0 - which * p.heads)) * p.tokens;
  const bool swapped = (lane >> 3) & 1;
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    lds_barrier();   // pass 0: every wave is done with the operand stages; later: the previous pass's chunk reads are done
#pragma unroll
    for (int i2 = 0; i2 < BLK; ++i2)
#pragma unroll
      for (int j = 0; j < G::MJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          ct[(wr * WR_ROWS + i2 * 16 + g * 4 + r) * CT_LD + wc * G::WN + j * 16 + c16] = acc[BLK * pass + i2][j][r] + bias[j];
    lds_barrier();
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      const int i = t + 512 * q;
      const int head = i / CHD, rem = i % CHD, row = rem / CPH, c = rem % CPH;
      const int grow = m0 + (row / WR_ROWS) * G::WM + pass * WR_ROWS + row % WR_ROWS;
      if (grow < M) {
        const float* src = ct + row * CT_LD + head * G::QKV_HD + NV * (c < DCH ? c : DCH - 1);
        const f32x4 first = *reinterpret_cast<const f32x4*>(src + (swapped ? 4 : 0));
        const f32x4 second = *reinterpret_cast<const f32x4*>(src + (swapped ? 0 : 4));
        int b, n;
        qkv_split_row(grow, p.tokens, b, n);
        const int drow = rows0 + (b * p.heads + head) * p.tokens + n;
        epi_qkv_halves<TOut>(first, second, swapped, c >= DCH,
                             reinterpret_cast<TOut*>(p.out) + (size_t)drow * G::QKV_HDP + NV * c);
      }
    }
  }
}

// blockIdx -> work unit.  Workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8 labels the XCD group), each
// with a private 4 MiB L2.  XCD x takes the CONTIGUOUS chunk [x*per, (x+1)*per) of a locality-ordered unit list, so
// the ~32 workgroups it runs at any moment are neighbours in that list.  Speed only; any placement is correct.
__device__ __forceinline__ int unit_of_block(int bid, int per) { return (bid & 7) * per + (bid >> 3); }

// NT tile order: bands of 8 row-tiles, column-major inside a band ("grouped" order): 32 consecutive tiles form an
// 8 x 4 block of the tile grid, i.e. 8 A panels + 4 B panels feed 32 tiles out of one L2.
__device__ __forceinline__ void tile_of_unit(int u, int tiles_m, int tiles_n, int& tile_m, int& tile_n, int bh = 8) {
  const int band = u / (bh * tiles_n);
  const int rows = (tiles_m - band * bh < bh) ? tiles_m - band * bh : bh;
  const int r = u - band * bh * tiles_n;
  tile_n = r / rows;
  tile_m = band * bh + (r - tile_n * rows);
}

// "B-stationary" alternative (band_h < 0 selects it, column-group width = -band_h): XCD x owns the contiguous range of row
// tiles [x*tiles_m/8, (x+1)*tiles_m/8) and walks it once per group of `cgw` column tiles — column group outermost, then
// rows, then the group's columns.  The ~32 workgroups an XCD runs at once are then (32/cgw) rows x cgw columns, and the
// NEXT 32 reuse the same cgw weight panels (4 x 590 KB at K = 1152: they stay in the XCD's 4-MiB L2) while only the
// activation panels stream: per 32 tiles 8 panel fetches instead of 12.  blockIdx b -> (XCD b & 7, local index b >> 3).
__device__ __forceinline__ bool tile_of_local(int xcd, int v, int tiles_m, int tiles_n, int cgw, int& tm, int& tn) {
  const int r_lo = (xcd * tiles_m) >> 3, r_hi = ((xcd + 1) * tiles_m) >> 3;
  const int R = r_hi - r_lo;
  if (v >= R * tiles_n) return false;
  const int full = R * cgw;
  const int g = v / full, rem = v - g * full;
  const int w = (tiles_n - g * cgw < cgw) ? tiles_n - g * cgw : cgw;
  const int r = rem / w;
  tm = r_lo + r;
  tn = g * cgw + (rem - r * w);
  return true;
}

// ------------------------------------------------------------------------------------------------------
// Anti-phase ("ping-pong") main loops, generation 6.  The two wave groups of the workgroup (G0 = waves
// 0-3, G1 = waves 4-7; every SIMD holds one wave of each) alternate: time is cut into slots separated by workgroup
// barriers, and in every slot one group issues the LDS reads of its next half K-step (plus its share of the
// global->LDS DMA stream) while the other group issues its MFMAs, so each SIMD's matrix pipe always has exactly one
// wave feeding it and nobody's LDS latency is exposed.  G1 simply starts one barrier late.  Measured against the
// generation-2 loop (one barrier per K-step, rolling fragment prefetch; since removed) in the same process: +8..14 % on the
// encoder's NT shapes, 1.29 -> 1.45 PFLOP/s at 8192^3.  Variants tried and dropped: 8 slots of 16 MFMAs (+4 %; the
// barrier hand-off costs about as much per slot regardless of slot length), 2 slots of 64 MFMAs (needs all DMA
// issued one slot before use: the prefetch distance is too short, -12 %).
//
// LDS-DMA is issued through inline asm: with the builtin the compiler cannot prove that a ds_read_b64_tr_b16 does not
// alias the in-flight DMA and drains vmcnt(0) in front of every transposed read.  The kernels own the vmcnt
// accounting instead: every read slot ends with pp_end_read<NI>(), NI the DMA instructions of a wave per K-step.
__device__ __forceinline__ void pp_dma16(u32x4 desc, uint32_t lds_addr, uint32_t voff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
               :: "s"(lds_addr), "v"(voff), "s"(desc) : "memory");
}
__device__ __forceinline__ u32x4 pp_desc(const void* base, uint32_t bytes) {
  const uint64_t q = (uint64_t)base;
  u32x4 d = {(uint32_t)q, (uint32_t)(q >> 32) & 0xffffu, bytes, 0x00020000u};
  return d;
}
// a descriptor whose words the compiler cannot prove wave-uniform (it must sit in SGPRs for the "s" operand above)
__device__ __forceinline__ u32x4 pp_desc_sgpr(u32x4 d) {
  return u32x4{(uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]), (uint32_t)__builtin_amdgcn_readfirstlane((int)d[1]),
               (uint32_t)__builtin_amdgcn_readfirstlane((int)d[2]), (uint32_t)__builtin_amdgcn_readfirstlane((int)d[3])};
}
// end of a read slot: all but the NI youngest DMA instructions of this wave have landed, its fragment reads are done
template <int NI>
__device__ __forceinline__ void pp_end_read() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(NI) : "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}
#define SGL_PP_END_MFMA()                 \
  do {                                    \
    __builtin_amdgcn_sched_barrier(0);    \
    __builtin_amdgcn_s_barrier();         \
    __builtin_amdgcn_sched_barrier(0);    \
  } while (0)

// Developer build (make TIMELINE=1, then SGL_TIMELINE=1 in the environment): s_memtime stamps at kernel entry, end of the
// main loop and end of the epilogue, summed over all workgroups and printed per launch.  This is the tool behind the
// epilogue findings of DESIGN.md section 8.4, round 2 (loads queued behind stores; fc1's main loop slowed by its own output traffic).
#ifdef SGL_TIMELINE
__device__ unsigned long long g_nt6_tl[4];
__device__ unsigned long long g_tn6_tl[12];   // [group][phase 0..4, slot-pair count]
#define SGL_TL_STAMP(v) const unsigned long long v = __builtin_readcyclecounter()
#else
#define SGL_TL_STAMP(v)
#endif

// NT on a tile geometry G, four slots per K-step.  The global->LDS stream moves three units per K-step in the fixed
// round-robin order
//     A0(t) = the first WM/2 rows of every wave row,  B(t) = all BN columns,  A1(t) = the other WM/2 rows,  A0(t+1), ...
// of P0, P1 and P2 = P0 wave-instructions per wave (NI = P0 + P1 + P2 per K-step).  Piece P0 w + q of A0 / A1 covers image rows
// WM (piece / ppw) + 8 (piece % ppw) (+ WM/2 for A1), ppw = WM/16 pieces per wave row; the B pieces are G::b_row.
// Per wave and K-step t, with HI = MI/2:
//     R1(t): fragment reads of B (MJ column blocks) and A0 (row blocks 0..HI-1), both k-halves   + DMA unit A1(t+1)
//     M1(t): A0 x B   2 HI MJ MFMAs (k-half 0 of all HI MJ accumulators, then k-half 1)
//     R2(t): fragment reads of A1 (row blocks HI..MI-1), both k-halves                           + DMA units A0(t+2), B(t+2)
//     M2(t): A1 x B   2 HI MJ MFMAs
// G0 runs R1 in slot 4t, G1 in slot 4t+1.  Every accumulator sees K-steps ascending, k-half 0 then 1, in one MFMA chain,
// whatever the geometry: the tiles agree bit for bit (tests/test_gemm_nt_384_gpu.py).  Every read slot ends with
// s_waitcnt vmcnt(NI): after R1(t) the NI younger instructions are A0(t+1), B(t+1), A1(t+1), so A1(t) has landed for
// R2(t); after R2(t) they are A1(t+1), A0(t+2), B(t+2), so A0(t+1) and B(t+1) have landed for R1(t+1).  Invariants
// (DESIGN.md section 4a):
//   (a) a unit is issued at least 4 slots = one K-step before the wait that publishes it;
//   (b) both groups have passed that wait and a barrier before anyone reads it;
//   (c) a unit is issued only after both groups finished (lgkmcnt(0) + barrier) reading the unit it overwrites:
//       A1(t+1) over A1(t-1), last read in slot 4t-1, issued from slot 4t; A0/B(t+2) over A0/B(t), last read in slot
//       4t+1, issued from slot 4t+2;
//   (d) every wave passes 4 barriers per K-step + 2 whatever its `active` state or group.
// A geometry with SPLIT_B reads B in halves instead (NtTile288: A in halves would put 22 fragment reads into R1 and 4
// into R2).  The three units, in the same round-robin order and the same slots, are then
//     A(t) = all BM rows,  B0(t) = column blocks 0..J0-1 of every wave column (+ the image's pad rows),  B1(t) = the other J1,
// of P0, P1 and P2 wave-instructions per wave (the same for every wave: the pad rows even B0 out), and
//     R1(t): fragment reads of A (all MI row blocks) and B0, both k-halves     + DMA unit B1(t+1)
//     M1(t): A x B0   2 MI J0 MFMAs
//     R2(t): fragment reads of B1, both k-halves; A stays in its registers      + DMA units A(t+2), B0(t+2)
//     M2(t): A x B1   2 MI J1 MFMAs
// i.e. the schedule above with (A0, B, A1) -> (A, B0, B1): what R1 reads is units 0 and 1, what R2 reads is unit 2.  The
// waits are the same: after R1(t) the NI younger instructions are A(t+1), B0(t+1), B1(t+1), so B1(t) has landed for R2(t);
// after R2(t) they are B1(t+1), A(t+2), B0(t+2), so A(t+1) and B0(t+1) have landed for R1(t+1).  The invariants, re-derived:
//   (a) B1(t+1) is issued in R1(t) and published by the wait of R1(t+1); A/B0(t+2) in R2(t), published by R2(t+1): 4 slots;
//   (b) as above: the publishing wait is followed by the read slot's barrier, and the reading slot of either group
//       comes at least one barrier after the later group's wait;
//   (c) B1(t+1) overwrites B1(t-1), last read in R2(t-1) (G1: slot 4t-1), issued from slot 4t; A/B0(t+2) overwrite A/B0(t),
//       last read in R1(t) (G1: slot 4t+1), issued from slot 4t+2.  A's registers are read by M2(t) after the stage's A
//       image may already be overwritten by A(t+2): they were loaded in R1(t), the image is not read again;
//   (d) unchanged: the slot structure is the same.
// Accumulator (i, j) is touched by M1 only (j < J0) or by M2 only, k-half 0 then 1: the chain order is the same.
//              tile       waves   MI x MJ   P0  P1  P2  NI = vmcnt   reads R1 / R2   MFMAs M1 / M2   LDS
//   NtTile256  256 x 256  2 x 4   8 x 4     2   4   2   8            16 / 8          32 / 32         128 KiB
//   NtTile384  384 x 192  4 x 2   6 x 6     3   3   3   9            18 / 6          36 / 36         144 KiB
//   NtTile288  256 x 288  4 x 2   4 x 9     4   3   2   9            18 / 8          40 / 32         144 KiB   (SPLIT_B)
// Operands are reached only through the two bounded buffer descriptors (rows past M / N and k past K come back as
// zeros), so ragged M, N and K need no branches.
// Two other schedules were measured on NtTile384 at M = 93,312, N = 1152, K = 4352 (NtTile256: 766 us): splitting the
// K-step by k-half (12 fragments live instead of 18, 12 + 12 reads) frees a stage only as a whole, so all nine DMA
// instructions of a wave fall into one slot, three slots before their wait: 900 us; this schedule: 711 us; this schedule
// with A1(t+1) issued from the MFMA slot that runs beside the other group's R1: 749 us.
template <typename G, int EPI, typename TOut, typename TIn>
__global__ __launch_bounds__(512, 2) void gemm_nt6_kernel(const TIn* __restrict__ A, int lda,
                                                          const TIn* __restrict__ B, int ldb, int M, int N, int K,
                                                          int tiles_m, int tiles_n, int band_h, EpiParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SGL_TL_STAMP(tl0);
  const int ntiles = tiles_m * tiles_n;
  int tile_m, tile_n;
  if (band_h < 0) {
    if (!tile_of_local(blockIdx.x & 7, blockIdx.x >> 3, tiles_m, tiles_n, -band_h, tile_m, tile_n)) return;
  } else {
    const int unit = unit_of_block(blockIdx.x, (ntiles + 7) >> 3);
    if (unit >= ntiles) return;  // whole block exits together
    tile_of_unit(unit, tiles_m, tiles_n, tile_m, tile_n, band_h);
  }
  constexpr int MI = G::MI, MJ = G::MJ, HI = MI / 2, J0 = G::J0, J1 = G::J1, NI = G::NI;
  constexpr bool SB = G::SPLIT_B;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = G::wr(w), wc = G::wc(w), grp = w >> 2;
  const int m0 = tile_m * G::BM, n0 = tile_n * G::BN;
  const int rows_a = (M - m0 < G::BM) ? M - m0 : G::BM;
  const int rows_b = (N - n0 < G::BN) ? N - n0 : G::BN;
  const u32x4 da = pp_desc(A + (size_t)m0 * lda, (uint32_t)(((size_t)(rows_a - 1) * lda + K) * 2));
  const u32x4 db = pp_desc(B + (size_t)n0 * ldb, (uint32_t)(((size_t)(rows_b - 1) * ldb + K) * 2));
  const uint32_t lds0 = (uint32_t)(size_t)((SGL_LDS char*)smem);

  // DMA plan: per unit and instruction the lane's source offset and the instruction's LDS address
  // units in stream order: U0 and U1 are read in R1, U2 in R2 (A0, B, A1; with SPLIT_B: A, B0, B1)
  constexpr int PU[3] = {G::P0, G::P1, G::P2};
  constexpr int PMAX = G::P0 > G::P1 ? (G::P0 > G::P2 ? G::P0 : G::P2) : (G::P1 > G::P2 ? G::P1 : G::P2);
  const int drow = lane >> 3, dchunk = (lane & 7) ^ drow;
  uint32_t voff[3][PMAX], ldst[3][PMAX];
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int q = 0; q < PU[u]; ++q) {
      const bool isA = SB ? u == 0 : u != 1;
      int r0;
      if constexpr (SB) {
        r0 = isA ? 8 * (G::P0 * w + q) : G::b_row(w, u - 1, q);
      } else {
        constexpr int ppw = G::WM / 16;
        const int piece = G::P0 * w + q;
        r0 = isA ? G::WM * (piece / ppw) + 8 * (piece % ppw) + (u == 2 ? G::WM / 2 : 0) : G::b_row(w, q);
      }
      const int row = r0 + drow;
      voff[u][q] = (row < (isA ? rows_a : rows_b)) ? (uint32_t)(row * (isA ? lda : ldb) + dchunk * 8) * 2u : SGL_OOB;
      ldst[u][q] = lds0 + (isA ? 0 : G::OPA) + (uint32_t)r0 * 128u;
    }
  const int nk = (K + T_BK - 1) / T_BK;
  auto issue = [&](int u, int kt) {  // unit u of K-step kt (K-steps past the end: all lanes out of range -> zeros)
    const int k0 = kt * T_BK;
    const bool kok = (kt < nk) && (k0 + dchunk * 8 < K);
    const uint32_t sb = (uint32_t)((kt & 1) * G::STAGE);
    const bool isA = SB ? u == 0 : u != 1;
#pragma unroll
    for (int q = 0; q < PU[u]; ++q)
      pp_dma16(isA ? da : db, ldst[u][q] + sb, (kok && voff[u][q] != SGL_OOB) ? voff[u][q] + (uint32_t)k0 * 2u : SGL_OOB);
  };

  const int frow = lane & 15, fg = lane >> 4, fsw = frow & 7;
  const uint32_t fa_base = (uint32_t)((wr * G::WM + frow) * 128);
  const uint32_t fb_base = (uint32_t)(G::OPA + (wc * G::WN + frow) * 128);
  const uint32_t c0 = (uint32_t)(((0 + fg) ^ fsw) << 4), c1 = (uint32_t)(((4 + fg) ^ fsw) << 4);
  const bool active = (n0 + wc * G::WN < N) && (m0 + wr * G::WM < M);

  f32x4 acc[MI][MJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0, 0); issue(1, 0); issue(2, 0);
  issue(0, 1); issue(1, 1);
  pp_end_read<NI>();                 // U0(0), U1(0) of every wave have landed
  if (grp == 1) SGL_PP_END_MFMA();   // G1 runs one slot behind G0 from here on

  // the fragments of one slot, [k-half][block]: NA row blocks of A, NB column blocks of B (SPLIT_B: all of A stays live
  // from R1 to M2 and B changes; otherwise all of B stays and A changes)
  constexpr int NA = SB ? MI : HI, NB = SB ? J0 : MJ;
  lo_x8<TIn> fa[2 * NA], fb[2 * NB];
  // M1 (half 0) / M2 (half 1): row blocks i0..i0+ni-1 x column blocks j0..j0+nj-1.  Order: k-half, row block, column block
  // (do not reorder: it is what makes the geometries agree bit for bit)
  auto mfma_slot = [&](auto half) {
    constexpr int hf = decltype(half)::value;
    constexpr int i0 = SB ? 0 : hf * HI, ni = SB ? MI : HI;
    constexpr int j0 = SB ? hf * J0 : 0, nj = SB ? (hf ? J1 : J0) : MJ;
    if (active) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < ni; ++i)
#pragma unroll
          for (int j = 0; j < nj; ++j)
            acc[i0 + i][j0 + j] = mfma_16x16x32(fa[ni * h + i], fb[nj * h + j], acc[i0 + i][j0 + j]);
      __builtin_amdgcn_s_setprio(0);
    }
    SGL_PP_END_MFMA();
  };
  for (int kt = 0; kt < nk; ++kt) {
    const char* base = smem + (kt & 1) * G::STAGE;
    const char* pa = base + fa_base;
    const char* pb = base + fb_base;
    // ---- R1: B and A0 (SPLIT_B: B0 and A)
    if (active) {
#pragma unroll
      for (int f = 0; f < 2 * NB; ++f) fb[f] = *reinterpret_cast<const lo_x8<TIn>*>(pb + (f % NB) * 2048 + ((f / NB) ? c1 : c0));
#pragma unroll
      for (int f = 0; f < 2 * NA; ++f) fa[f] = *reinterpret_cast<const lo_x8<TIn>*>(pa + (f % NA) * 2048 + ((f / NA) ? c1 : c0));
    }
    issue(2, kt + 1);
    pp_end_read<NI>();
    mfma_slot(std::integral_constant<int, 0>{});
    // ---- R2: A1 (SPLIT_B: B1)
    if (active) {
      if constexpr (SB) {
#pragma unroll
        for (int f = 0; f < 2 * J1; ++f) fb[f] = *reinterpret_cast<const lo_x8<TIn>*>(pb + (J0 + f % J1) * 2048 + ((f / J1) ? c1 : c0));
      } else {
#pragma unroll
        for (int f = 0; f < 2 * HI; ++f) fa[f] = *reinterpret_cast<const lo_x8<TIn>*>(pa + (HI + f % HI) * 2048 + ((f / HI) ? c1 : c0));
      }
    }
    issue(0, kt + 2); issue(1, kt + 2);
    pp_end_read<NI>();
    mfma_slot(std::integral_constant<int, 1>{});
  }
  if (grp == 0) SGL_PP_END_MFMA();   // G0 waits for G1's last slot
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing (all-zero) units must land before the LDS is reused
#ifdef SGL_TIMELINE
  if (p.atomic == 77) return;   // developer build only (SGL_NT6_SKIP_EPI): main loop without its epilogue
#endif
  SGL_TL_STAMP(tl1);
  if constexpr (EPI == EPI_QKV && G::QKV_HD > 0)
    store_tile_qkv_heads<G, TOut>(smem, acc, wr, wc, lane, t, m0, n0, M, p);
  else
    store_tile_pp<G, EPI, TOut>(smem, acc, wr, wc, lane, t, m0, n0, M, N, p);
#ifdef SGL_TIMELINE
  SGL_TL_STAMP(tl2);
  if (t == 0) {
    atomicAdd(&g_nt6_tl[0], tl1 - tl0);
    atomicAdd(&g_nt6_tl[1], tl2 - tl1);
    atomicAdd(&g_nt6_tl[2], 1ull);
  }
#endif
}

// ------------------------------------------------------------------------------------------------------
// TN (dW) on a tile geometry G, four slots per K-step of 64 tokens, split by K-HALF: the token index is the MFMA k
// index, so the first 32 image rows of both operands feed the first MI MJ MFMAs (every accumulator once) and the last
// 32 rows the other MI MJ.
//     R1(t): k-half 0 fragments (MI of A + MJ of B, two transposed reads each) + DMA unit H1(t+1)
//     M1(t): MI MJ MFMAs      R2(t): k-half 1 fragments + DMA unit H0(t+2)      M2(t): MI MJ MFMAs
// Unit Hh = image rows 32h..32h+31 of A, then of B.  Both images are token rows of RA = 2 BM and RB = 2 BN bytes, a
// k-half of them HA = BM/16 and HB = BN/16 contiguous KiB, one DMA instruction each: wave w moves A pieces PA w + q
// (PA = HA/8) and B pieces PB w + q (PB = HB/8); where HB is 8 PB + 4 (the 192-wide image: 12 pieces) the four waves of
// group h also move piece 8 PB + (w & 3) of Hh.  Every wave then issues the same NI = 2 PA + 2 PB (+ 1) instructions per
// K-step, in whichever two slots, and every read slot ends with vmcnt(NI): behind the unit it publishes a wave has
// issued exactly the two younger units, one of each k-half, i.e. NI instructions (pipeline start: H0(0), H1(0), H0(1)
// issued, the same wait publishes H0(0)).  Invariants (a)-(d) of the NT loop hold with "unit" = Hh.
// Swizzle (tn_swz, chunks of 16 B): a 32-lane half of a transposed read touches 8 token rows {8g + q} x 32 B, which
// must fall into 8 different 32-B bank groups of the 256-B bank row.  Rows of 0 mod 256 bytes (512: 256 columns, 768:
// 384 columns) all start on bank 0: slot s of row m holds chunk s ^ (2 (m & 3) + 8 ((m >> 3) & 1)), closed inside every
// 256 B of the row.  Rows of 128 mod 256 bytes (384: 192 columns) already alternate between the two halves of the bank
// row with m & 1, and the pattern must stay inside 128 B: chunk s ^ (2 ((m >> 1) & 1) + 4 ((m >> 3) & 1)).
//              tile       MI x MJ   HA  HB   PA  PB(+1)  NI = vmcnt   reads per slot   MFMAs per slot   LDS
//   NtTile256  256 x 256  8 x 4     16  16   2   2       8            24               32               128 KiB
//   NtTile384  384 x 192  6 x 6     24  12   3   1 + 1   9            24               36               144 KiB
// Every accumulator sees K-steps ascending, k-half 0 then 1, in one MFMA chain on either geometry: with equal split
// boundaries the tiles agree bit for bit (tests/test_gemm_tn_384_gpu.py).
template <int ROWB>
__device__ __forceinline__ int tn_swz(int m) {
  static_assert(ROWB % 128 == 0, "the patterns are closed inside 256 / 128 bytes of a row");
  if constexpr (ROWB % 256 == 0) return 2 * (m & 3) + 8 * ((m >> 3) & 1);
  else return 2 * ((m >> 1) & 1) + 4 * ((m >> 3) & 1);
}

// Units are numbered split-major, tile2 fastest inside a split; an XCD runs a chunk of ~32 consecutive units at once
// (unit_of_block).  On a grid with few row tiles (fc2 dW: 5 x 17 tiles) that chunk is 1.9 x 17 tiles, 19-20 operand
// column slices through one L2 where 17 x 5 gives 11-12, and FETCH_SIZE shows it (+34 %); running the shorter grid side
// fastest removes the extra fills but moves no launch time out of its run-to-run band, so the
// order stays as it is.
template <typename G, typename TIn>
__global__ __launch_bounds__(512, 2) void gemm_tn6_kernel(const TIn* __restrict__ A, int lda,
                                                          const TIn* __restrict__ B, int ldb, int Mred, int N1, int N2,
                                                          int m_per_split, int nsplits, int tiles_1, int tiles_2,
                                                          EpiParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int MI = G::MI, MJ = G::MJ;
  constexpr int RA = 2 * G::BM, RB = 2 * G::BN;            // bytes of a token row of the A / B image
  constexpr int HA = G::BM / 16, HB = G::BN / 16;          // 1-KiB pieces of a k-half
  constexpr int PA = HA / 8, PB = HB / 8;
  constexpr bool BX = (HB % 8) != 0;                       // four pieces over: one more for each wave of group h
  constexpr int NI = 2 * PA + 2 * PB + (BX ? 1 : 0);
  static_assert(HA % 8 == 0 && (HB % 8 == 0 || HB % 8 == 4), "pieces of a k-half over 8 waves (+ one wave group)");
  const int ntiles = tiles_1 * tiles_2;
  const int nunits = ntiles * nsplits;
  const int unit = unit_of_block(blockIdx.x, (nunits + 7) >> 3);
  if (unit >= nunits) return;
  const int split = unit / ntiles, trem = unit - split * ntiles;
  const int tile1 = trem / tiles_2, tile2 = trem - tile1 * tiles_2;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = G::wr(w), wc = G::wc(w), grp = w >> 2;
  const int n1_0 = tile1 * G::BM, n2_0 = tile2 * G::BN;
  const int m_begin = split * m_per_split;
  const int m_end = (m_begin + m_per_split < Mred) ? m_begin + m_per_split : Mred;
  const int rows = m_end - m_begin;
  const u32x4 da = pp_desc_sgpr(pp_desc(A + (size_t)m_begin * lda, (uint32_t)((size_t)rows * lda * 2)));
  const u32x4 db = pp_desc_sgpr(pp_desc(B + (size_t)m_begin * ldb, (uint32_t)((size_t)rows * ldb * 2)));
  const uint32_t lds0 = (uint32_t)(size_t)((SGL_LDS char*)smem);

  // DMA plan: lane l of piece c of unit Hh writes image bytes 1024 c + 16 l of the k-half, i.e. slot s of token row
  // 32 h + r, and fetches the chunk that the swizzle puts there
  uint32_t voffA[2][PA], ldsA[2][PA], voffB[2][PB + 1], ldsB[2][PB + 1];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < PA; ++q) {
      const int piece = PA * w + q, pos = 1024 * piece + 16 * lane;
      const int row = 32 * h + pos / RA, chunk = ((pos % RA) >> 4) ^ tn_swz<RA>(row);
      const int col = n1_0 + chunk * 8;
      voffA[h][q] = (col < N1) ? (uint32_t)(row * lda + col) * 2u : SGL_OOB;
      ldsA[h][q] = lds0 + (uint32_t)(h * 32 * RA + 1024 * piece);
    }
#pragma unroll
    for (int q = 0; q < PB + 1; ++q) {
      const int piece = (q < PB) ? PB * w + q : 8 * PB + (w & 3), pos = 1024 * piece + 16 * lane;
      const int row = 32 * h + pos / RB, chunk = ((pos % RB) >> 4) ^ tn_swz<RB>(row);
      const int col = n2_0 + chunk * 8;
      voffB[h][q] = (col < N2) ? (uint32_t)(row * ldb + col) * 2u : SGL_OOB;
      ldsB[h][q] = lds0 + (uint32_t)(G::OPA + h * 32 * RB + 1024 * piece);
    }
  }
  auto issue = [&](int h, int kt) {  // rows past the split's range are out of range for the descriptor -> zeros
    const uint32_t r0 = (uint32_t)kt * T_BK;
    const uint32_t sb = (uint32_t)((kt & 1) * G::STAGE);
    const uint32_t adva = r0 * (uint32_t)lda * 2u, advb = r0 * (uint32_t)ldb * 2u;
#pragma unroll
    for (int q = 0; q < PA; ++q) pp_dma16(da, ldsA[h][q] + sb, voffA[h][q] == SGL_OOB ? SGL_OOB : voffA[h][q] + adva);
#pragma unroll
    for (int q = 0; q < PB; ++q) pp_dma16(db, ldsB[h][q] + sb, voffB[h][q] == SGL_OOB ? SGL_OOB : voffB[h][q] + advb);
    if constexpr (BX) {
      if (grp == h) pp_dma16(db, ldsB[h][PB] + sb, voffB[h][PB] == SGL_OOB ? SGL_OOB : voffB[h][PB] + advb);
    }
  };

  // fragment block i (16 columns = 32 B) of this wave: token row 8 fg + fq (and + 4), 8 B at column block + 4 fp
  const int fg = lane >> 4, fq = (lane >> 2) & 3, fp = lane & 3;
  const int fm = 8 * fg + fq;
  uint32_t fa_off[MI], fb_off[MJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
    fa_off[i] = (uint32_t)(fm * RA) + ((uint32_t)(wr * G::WM * 2 + i * 32 + 8 * fp) ^ (uint32_t)(16 * tn_swz<RA>(fm)));
#pragma unroll
  for (int j = 0; j < MJ; ++j)
    fb_off[j] = (uint32_t)(G::OPA + fm * RB) + ((uint32_t)(wc * G::WN * 2 + j * 32 + 8 * fp) ^ (uint32_t)(16 * tn_swz<RB>(fm)));
  const bool active = (n2_0 + wc * G::WN < N2) && (n1_0 + wr * G::WM < N1);

  f32x4 acc[MI][MJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (rows + T_BK - 1) / T_BK;
  issue(0, 0); issue(1, 0);
  issue(0, 1);
  pp_end_read<NI>();                 // H0(0) of every wave has landed
  if (grp == 1) SGL_PP_END_MFMA();   // G1 runs one slot behind G0 from here on

#define SGL_TR6(ptr, rowb) \
  __builtin_shufflevector(lds_read_tr16<TIn>(ptr), lds_read_tr16<TIn>((ptr) + 4 * (rowb)), 0, 1, 2, 3, 4, 5, 6, 7)
  lo_x8<TIn> fa[MI], fb[MJ];
#ifdef SGL_TIMELINE
  // per-phase cycle sums of this wave over the main loop: [0] issue fragment reads + DMA, [1] wait for them (lgkmcnt/vmcnt),
  // [2] barrier after the read slot, [3] the slot's MFMAs, [4] barrier after the MFMA slot
  unsigned long long tlp[5] = {0, 0, 0, 0, 0};
#define SGL_TLP(i) do { const unsigned long long n_ = __builtin_readcyclecounter(); tlp[i] += n_ - tl_last; tl_last = n_; } while (0)
  unsigned long long tl_last = __builtin_readcyclecounter();
#else
#define SGL_TLP(i)
#endif
  for (int kt = 0; kt < nk; ++kt) {
    const char* base = smem + (kt & 1) * G::STAGE;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (active) {
#pragma unroll
        for (int j = 0; j < MJ; ++j) fb[j] = SGL_TR6(base + h * 32 * RB + fb_off[j], RB);
#pragma unroll
        for (int i = 0; i < MI; ++i) fa[i] = SGL_TR6(base + h * 32 * RA + fa_off[i], RA);
      }
      if (h == 0) issue(1, kt + 1);
      else issue(0, kt + 2);
#ifdef SGL_TIMELINE
      SGL_TLP(0);
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(NI) : "memory");
      SGL_TLP(1);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      SGL_TLP(2);
#else
      pp_end_read<NI>();
#endif
      if (active) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < MJ; ++j)
            acc[i][j] = mfma_16x16x32(fa[i], fb[j], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
      }
#ifdef SGL_TIMELINE
      asm volatile("s_nop 0" ::"v"(acc[0][0]), "v"(acc[MI - 1][MJ - 1]));
      SGL_TLP(3);
#endif
      SGL_PP_END_MFMA();
      SGL_TLP(4);
    }
  }
#ifdef SGL_TIMELINE
  if (lane == 0 && active && (w == 0 || w == 4)) {
    for (int i = 0; i < 5; ++i) atomicAdd(&g_tn6_tl[(w >> 2) * 6 + i], tlp[i]);
    atomicAdd(&g_tn6_tl[(w >> 2) * 6 + 5], (unsigned long long)(2 * nk));
  }
#endif
#undef SGL_TR6
  if (grp == 0) SGL_PP_END_MFMA();   // G0 waits for G1's last slot
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing (all-zero) units must land before the LDS is reused
  EpiParams pq = p;
  if (p.split_stride) pq.out = reinterpret_cast<float*>(p.out) + (size_t)split * p.split_stride;  // private slab of this split
  store_tile_pp<G, EPI_F32, float>(smem, acc, wr, wc, lane, t, n1_0, n2_0, N1, N2, pq);
}

// ------------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------------
#ifdef SGL_TIMELINE
// SGL_TIMELINE=1 in the environment: wait for the launch, hand the kernel's counters to `print`, clear them.
// Synchronises: measurement builds only.
template <int NC, typename Print>
static void timeline_report(hipStream_t s, unsigned long long (&counters)[NC], Print&& print) {
  if (!getenv("SGL_TIMELINE")) return;
  unsigned long long h[NC];
  (void)hipStreamSynchronize(s);
  (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(counters), sizeof(h));
  print(h);
  memset(h, 0, sizeof(h));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(counters), h, sizeof(h));
}
#endif

template <typename G, int EPI, typename TOut, typename TIn>
static hipError_t launch_nt_pp(const TIn* A, int lda, const TIn* B, int ldb, int M, int N, int K, const EpiParams& p,
                               hipStream_t s) {
  const hipError_t e = set_max_dynamic_lds_once<&gemm_nt6_kernel<G, EPI, TOut, TIn>>(G::LDS);
  if (e != hipSuccess) return e;
  const int tiles_m = (M + G::BM - 1) / G::BM, tiles_n = (N + G::BN - 1) / G::BN;
  // Tile order.  Default (round 2): B-stationary with column groups of 8 — same speed as the round-1 grouped bands
  // (+-1 % over the encoder's eight shapes) but 35 % fewer bytes leave the XCD L2s at the bench batch (rocprofv3
  // FETCH_SIZE: 2.42 -> 1.56 GB per fc1 launch at B = 128, profiles/r02_pmc_traffic.json); on NtTile384 an XCD walks
  // its 30-31 row tiles with all six column tiles of an output 1152 wide in one column group.  SGL_BAND > 0 selects the
  // grouped bands of that height (8 / 4 were the round-1 choices: measured on one box, qkv N=3456 +3 %, fc2 N=1152
  // +1.5 % with 4; fc1 N=4352 best with 8), SGL_BAND < 0 another column-group width.
  static const int band_env = getenv("SGL_BAND") ? atoi(getenv("SGL_BAND")) : 0;
  const int band_h = band_env != 0 ? band_env : -8;
  const int grid = band_h < 0 ? 8 * (((tiles_m + 7) / 8) * tiles_n)     // 8 XCDs x the largest per-XCD tile count
                              : ((tiles_m * tiles_n + 7) / 8) * 8;      // one workgroup per tile, whole XCD rounds
  EpiParams pp = p;
#ifdef SGL_TIMELINE   // measurement builds only (make TIMELINE=1): the product library never skips an epilogue
  static const bool skip_epi = getenv("SGL_NT6_SKIP_EPI") != nullptr;
  if (skip_epi && EPI != EPI_F32) pp.atomic = 77;
#endif
  hipLaunchKernelGGL((gemm_nt6_kernel<G, EPI, TOut, TIn>), dim3(grid), dim3(512), G::LDS, s, A, lda, B, ldb, M, N, K,
                     tiles_m, tiles_n, band_h, pp);
#ifdef SGL_TIMELINE
  timeline_report(s, g_nt6_tl, [&](const unsigned long long* h) {
    if (h[2])
      fprintf(stderr, "[timeline] gemm_nt6 %dx%d EPI %d M=%d N=%d K=%d: %llu tiles, main loop %.0f, epilogue %.0f cycles per tile\n",
              G::BM, G::BN, EPI, M, N, K, h[2], (double)h[0] / h[2], (double)h[1] / h[2]);
  });
#endif
  return hipGetLastError();
}

// every (epilogue, output type) pair of dispatch_epilogue that the geometry takes
template <typename G, typename TIn>
static hipError_t gemm_nt_pp(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                             const EpiParams& p, hipStream_t s) {
  return dispatch_epilogue<TIn>(epi, out_dtype, [&](auto tag) {
    using T = decltype(tag);
    if constexpr (G::takes(T::epi) && (G::QKV_HD == 0 || sizeof(typename T::out) == 2))
      return launch_nt_pp<G, T::epi, typename T::out, TIn>((const TIn*)A, lda, (const TIn*)B, ldb, M, N, K, p, s);
    else
      return hipErrorInvalidValue;
  });
}
template <typename TIn>
hipError_t gemm_nt256(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                      const EpiParams& p, hipStream_t s) {
  return gemm_nt_pp<NtTile256, TIn>(A, lda, B, ldb, M, N, K, epi, out_dtype, p, s);
}
template <typename TIn>
hipError_t gemm_nt384(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                      const EpiParams& p, hipStream_t s) {
  return gemm_nt_pp<NtTile384, TIn>(A, lda, B, ldb, M, N, K, epi, out_dtype, p, s);
}
// heads of this many columns, stored this wide, make whole 288-column tiles (gemm_nt_mfma checks the rest)
static_assert(NtTile288::QKV_HD == NT288_HEAD_DIM && NtTile288::QKV_HDP == NT288_HEAD_DIM_PAD && NtTile288::BN == NT288_BN, "kernels.h");
template <typename TIn>
hipError_t gemm_nt288(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, int out_dtype,
                      const EpiParams& p, hipStream_t s) {
  // the head-major epilogue addresses with the geometry's constants: nothing else may reach it
  if (epi != EPI_QKV || !nt288_takes_qkv(N, p)) return hipErrorInvalidValue;
  return gemm_nt_pp<NtTile288, TIn>(A, lda, B, ldb, M, N, K, epi, out_dtype, p, s);
}

template <typename G, typename TIn>
static hipError_t launch_tn_pp(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int m_per,
                               int splits, const EpiParams& p, hipStream_t s) {
  const hipError_t e = set_max_dynamic_lds_once<&gemm_tn6_kernel<G, TIn>>(G::LDS);
  if (e != hipSuccess) return e;
  const int tiles_1 = (N1 + G::BM - 1) / G::BM, tiles_2 = (N2 + G::BN - 1) / G::BN;
  const int grid = ((tiles_1 * tiles_2 * splits + 7) / 8) * 8;
  hipLaunchKernelGGL((gemm_tn6_kernel<G, TIn>), dim3(grid), dim3(512), G::LDS, s, (const TIn*)A, lda, (const TIn*)B, ldb,
                     Mred, N1, N2, m_per, splits, tiles_1, tiles_2, p);
#ifdef SGL_TIMELINE
  timeline_report(s, g_tn6_tl, [&](const unsigned long long* h) {
    for (int g = 0; g < 2; ++g)
      if (h[g * 6 + 5])
        fprintf(stderr, "[timeline] gemm_tn6 %dx%d N1=%d N2=%d Mred=%d splits=%d group %d, cycles per slot pair (read slot + MFMA slot): "
                "issue reads+DMA %.0f, wait %.0f, barrier %.0f, %d MFMAs %.0f, barrier %.0f\n", G::BM, G::BN, N1, N2, Mred, splits, g,
                (double)h[g * 6 + 0] / h[g * 6 + 5], (double)h[g * 6 + 1] / h[g * 6 + 5], (double)h[g * 6 + 2] / h[g * 6 + 5],
                G::MI * G::MJ, (double)h[g * 6 + 3] / h[g * 6 + 5], (double)h[g * 6 + 4] / h[g * 6 + 5]);
  });
#endif
  return hipGetLastError();
}
template <typename TIn>
hipError_t gemm_tn256(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int m_per, int splits,
                      const EpiParams& p, hipStream_t s) {
  return launch_tn_pp<NtTile256, TIn>(A, lda, B, ldb, Mred, N1, N2, m_per, splits, p, s);
}
template <typename TIn>
hipError_t gemm_tn384(const void* A, int lda, const void* B, int ldb, int Mred, int N1, int N2, int m_per, int splits,
                      const EpiParams& p, hipStream_t s) {
  return launch_tn_pp<NtTile384, TIn>(A, lda, B, ldb, Mred, N1, N2, m_per, splits, p, s);
}

#define SGL_INSTANTIATE_PP(TIn)                                                                                        \
  template hipError_t gemm_nt256<TIn>(const void*, int, const void*, int, int, int, int, int, int, const EpiParams&,   \
                                      hipStream_t);                                                                    \
  template hipError_t gemm_nt384<TIn>(const void*, int, const void*, int, int, int, int, int, int, const EpiParams&,   \
                                      hipStream_t);                                                                    \
  template hipError_t gemm_nt288<TIn>(const void*, int, const void*, int, int, int, int, int, int, const EpiParams&,   \
                                      hipStream_t);                                                                    \
  template hipError_t gemm_tn256<TIn>(const void*, int, const void*, int, int, int, int, int, int, const EpiParams&,   \
                                      hipStream_t);                                                                    \
  template hipError_t gemm_tn384<TIn>(const void*, int, const void*, int, int, int, int, int, int, const EpiParams&,   \
                                      hipStream_t);
SGL_INSTANTIATE_PP(bf16)
SGL_INSTANTIATE_PP(f16)
#undef SGL_INSTANTIATE_PP

}  // namespace sgl
