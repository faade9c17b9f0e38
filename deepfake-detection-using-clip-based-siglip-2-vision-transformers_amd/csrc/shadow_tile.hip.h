// How one 64x64 tile of an fp32 matrix becomes its two compute-dtype weight shadows: the row-major copy
// dst[(r - row0) * ld + c] and, through an LDS transpose, the transposed copy dst_t[c * ld_t + (r - row0)], both in
// >= 128-byte row segments.  The single writer behind the two routes that must leave the same bytes in the shadow arena:
// the re-cast (elementwise.hip, cast_job_kernel) and the optimizer (optimizer.hip, adamw_tile).
//
// A 256-thread block owns the tile at (r0, c0); thread (tx, ty) = (t & 15, t >> 4) holds, for k = 0..3, the four values
// of row r0 + ty + 16k at columns c0 + 4tx .. +3.  Rows outside [row_lo, row_hi) and columns >= cols are never written.
#pragma once
#include "common.hip.h"

namespace sgl {

template <typename T>
struct ShadowTile {
  T* dst;        // row-major copy or null
  T* dst_t;      // transposed copy or null
  int ld, ld_t;
  int row_lo, row_hi, cols, row0;
  int r0, c0;
  T* lt;         // LDS image [64][66]

  // 16-row step k: the row-major store and the tile image (v = zeros where the caller holds no value)
  __device__ __forceinline__ void put(int k, const float (&v)[4]) const {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int r = r0 + ty + 16 * k, cc = c0 + tx * 4;
    T o4[4] = {cvt_to<T>(v[0]), cvt_to<T>(v[1]), cvt_to<T>(v[2]), cvt_to<T>(v[3])};
    if (dst && r >= row_lo && r < row_hi && cc < cols) {
      T* d = dst + (size_t)(r - row0) * ld + cc;
      if (cc + 3 < cols && ((((uintptr_t)d) & (4 * sizeof(T) - 1)) == 0)) {
        if constexpr (sizeof(T) == 2) {
          u32x2 w;
          __builtin_memcpy(&w, o4, 8);
          *reinterpret_cast<u32x2*>(d) = w;
        } else {
          u32x4 w;
          __builtin_memcpy(&w, o4, 16);
          *reinterpret_cast<u32x4*>(d) = w;
        }
      } else {
        for (int j = 0; j < 4 && cc + j < cols; ++j) d[j] = o4[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) lt[(ty + 16 * k) * 66 + tx * 4 + j] = o4[j];
  }

  // after the four put()s: output row = column c0 + oc, 16 consecutive elements = rows r0 + 16*seg .. +15
  __device__ __forceinline__ void put_transposed() const {
    if (!dst_t) return;
    __syncthreads();
    const int oc = threadIdx.x >> 2, seg = threadIdx.x & 3;   // 64 output rows x 4 segments of 16 elements
    if (c0 + oc >= cols) return;
    const int rb = r0 + seg * 16;
    T* drow = dst_t + (size_t)(c0 + oc) * ld_t + (rb - row0);
    T vals[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) vals[j] = lt[(seg * 16 + j) * 66 + oc];
    if (rb >= row_lo && rb + 15 < row_hi && ((((uintptr_t)drow) & 15) == 0)) {
      constexpr int PER = 16 / sizeof(T);   // 16 consecutive elements of one output row: 16-byte stores
#pragma unroll
      for (int q = 0; q < 16 / PER; ++q) {
        u32x4 w;
        __builtin_memcpy(&w, &vals[q * PER], 16);
        *reinterpret_cast<u32x4*>(drow + q * PER) = w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (rb + j >= row_lo && rb + j < row_hi) drow[j] = vals[j];
    }
  }
};

}  // namespace sgl
