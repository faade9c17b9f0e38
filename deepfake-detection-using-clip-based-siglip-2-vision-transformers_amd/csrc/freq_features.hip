// The app's 24-D frequency / SRM feature vector (appv3.py:1618-1728 extract_freq_vector, DETECT_USE_CLAHE off) of V
// windows onto B same-size uint8 NHWC sources: what detect_core feeds FreqMLP for each of its 9 crops and each grid cell.
// include/siglip_hip.h (sgl_op_freq_features) has the contract; tests/freq_ref.py restates every rule.
//
// Seven launches per 64 views, every grid (something, views) so that one image's 25 windows fill the device:
//   coef      2 x nv blocks    PIL's bicubic coefficients of both axes, per output index, in fp64 (below); twiddles, the
//                              tables' member counts (one block), zeroing
//   gray_h    rows x nv        luma + horizontal uint8 pass -> scratch (h x 256 bytes per view)
//   gray_v    256 x nv         vertical uint8 pass -> the 256 x 256 gray plane (scratch, and gray_out)
//   stats     16 x nv          SRM responses and two Haar levels as exact integers, int64 power sums (integer atomics)
//   fft_rows  64 x nv          256-point FFT of 4 rows per block (one wave each, Stockham radix 2 in LDS), in fp64
//   fft_cols  64 x nv          the same over 4 columns; F rounded to fp32, then |F|, log, phase reduced against the three
//                              index tables into 50 partial sums per block (fixed order) and the 50-bin phase histogram
//                              (integer atomics)
//   finalize  nv               partials summed in block order, the 24 values in double, optional standardisation
// The row-pass spectrum (1 MiB per view) goes through caller scratch and is read back once, from L2.  No float atomics:
// two calls give the same bits.
//
// Why the transform is fp64 and not fp32: the error of an fp32 FFT scales with the root-mean-square of the whole
// spectrum, which the DC term dominates, not with the bin.  For an up-scaled window most bins lie three to four orders
// below that, their phases move by 1e-3 rad and thousands of the 65536 samples come within reach of a histogram edge: the
// entropy could not be held to a bound derived from the formats (tests/test_freq_features_host.py recomputes both
// bounds: 5.2x the entropy cap and 12.8x the slope cap for fp32 on the gratings, under 0.03x for fp64).  The vendor's
// peak fp64 vector rate equals the unpacked fp32 one on this part (not measured here); what the transform costs is in
// profiles/freq_bench.json.  After it every bin carries its own fp32 rounding only.
//
// Coefficients: PIL builds them in C doubles with add, mul and div only and a sequential sum (Resample.c precompute_coeffs,
// bicubic a = -0.5), then rounds to 22-bit fixed point.  The coef kernel does the same operations in the same order in
// fp64 with contraction off; each is IEEE-exact on gfx950, so the integers are PIL's.  One thread = one output index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hip.h"
#include "kernels.h"
#include "siglip_hip.h"

namespace sgl {
namespace freq {

constexpr int kN = 256;                                  // the plane's side
constexpr int kChunk = 64;                               // views per launch, as the views op
constexpr int kMaxSide = 4096;                           // window side cap: 2 * 16 * 2 + 1 = 65 taps
constexpr int kTaps = 65;
constexpr int kBits = 22;                                // PIL's PRECISION_BITS for 8-bit pixels
constexpr int kBuckets = 39, kSectors = 8, kBins = 50;
constexpr int kCats = 3 + kBuckets + kSectors;           // float categories reduced by fft_cols: 50
constexpr int kColBlocks = kN / 4;                       // 64 partial rows per view
constexpr int kSums = 16;                                // int64: 8 Haar sum c^2, 2 SRM kernels x sum n, n^2, n^3, n^4

struct Win {                                             // a checked view: image, origin, extents
  int src, x0, y0, w, h;
};
struct WinChunk {
  Win v[kChunk];
};
struct Axis {                                            // one resample pass: first tap, tap count and the fixed-point weights
  int lo[kN], n[kN];                                     // of every output index; tap-major, so that the threads of a row
  int k[kTaps + 1][kN];                                  // (one per output index) read neighbouring words
};

// per-view-slot scratch layout (bytes); a slot is reused by the next chunk of 64 (stream order)
struct Layout {
  size_t tw, axes, inter, gray, spec, part, sums, hist, slot, total;
};
__host__ __device__ inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr size_t kCountsAt = 128 * sizeof(double2);      // members per bucket (39) and sector (8), counted once per launch group
constexpr size_t kHead = 2304;                           // up256(kCountsAt + 47 * sizeof(int))
__host__ __device__ inline Layout layout(int slots, int Hs) {
  Layout L;
  const size_t hcap = Hs < kMaxSide ? Hs : kMaxSide;
  L.tw = 0;                                              // double2[128] twiddles, then int[47] member counts: shared
  const size_t head = kHead;
  L.axes = 0;
  L.inter = L.axes + up256(2 * sizeof(Axis));
  L.gray = L.inter + up256(hcap * kN);
  L.spec = L.gray + (size_t)kN * kN;
  L.part = L.spec + (size_t)kN * kN * sizeof(double2);
  L.sums = L.part + up256((size_t)kColBlocks * kCats * sizeof(float));
  L.hist = L.sums + up256(kSums * sizeof(long long));
  L.slot = L.hist + up256(kBins * sizeof(int));
  L.total = head + (size_t)slots * L.slot;
  return L;
}
__device__ __forceinline__ unsigned char* slot_ptr(void* scratch, const Layout& L, int v) {
  return reinterpret_cast<unsigned char*>(scratch) + kHead + (size_t)v * L.slot;
}

// ---- coefficients ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double bicubic(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

__device__ __forceinline__ void pil_axis(int o, int in, Axis* out) {
#pragma clang fp contract(off)
  const double scale = (double)in / (double)kN;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs;
  const double center = (o + 0.5) * scale;
  const double ss = 1.0 / fs;
  int lo = (int)(center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + support + 0.5);
  if (hi > in) hi = in;
  int n = hi - lo;
  if (n > kTaps) n = kTaps;                              // cannot happen for in <= 4096; keeps k[] in bounds regardless
  double ww = 0.0;
  for (int j = 0; j < n; ++j) ww += bicubic((j + lo - center + 0.5) * ss);
  for (int j = 0; j < n; ++j) {
    double w = bicubic((j + lo - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    out->k[j][o] = w < 0 ? (int)(-0.5 + w * (double)(1 << kBits)) : (int)(0.5 + w * (double)(1 << kBits));
  }
  out->lo[o] = lo;
  out->n[o] = n;
}

__global__ __launch_bounds__(256) void coef_kernel(const WinChunk chunk, void* scratch, Layout L,
                                                   const unsigned char* __restrict__ geom) {
  __shared__ int cnt[kBuckets + kSectors];
  const int v = blockIdx.y, axis = blockIdx.x, t = threadIdx.x;
  unsigned char* slot = slot_ptr(scratch, L, v);
  const Win w = chunk.v[v];
  pil_axis(t, axis == 0 ? w.w : w.h, reinterpret_cast<Axis*>(slot + L.axes) + axis);
  if (axis == 0) {
    if (t < kSums) reinterpret_cast<long long*>(slot + L.sums)[t] = 0;
    if (t < kBins) reinterpret_cast<int*>(slot + L.hist)[t] = 0;
    if (v == 0 && t < 128) {                             // exp(-2 pi i t / 256), made in double
      double s, c;
      sincospi(-(double)t / 128.0, &s, &c);
      reinterpret_cast<double2*>(scratch)[t] = make_double2(c, s);
    }
  } else if (v == 0) {                                   // members per bucket and sector: constants of the tables
    if (t < kBuckets + kSectors) cnt[t] = 0;
    __syncthreads();
    for (int i = t; i < kN * kN; i += 256) {
      const int bucket = geom[65536 + i], sector = geom[131072 + i];
      if (bucket < kBuckets) atomicAdd(&cnt[bucket], 1);
      if (sector < kSectors) atomicAdd(&cnt[kBuckets + sector], 1);
    }
    __syncthreads();
    if (t < kBuckets + kSectors) reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(scratch) + kCountsAt)[t] = cnt[t];
  }
}

// ---- gray plane --------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kBits;                            // arithmetic shift, as PIL
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void gray_h_kernel(const unsigned char* __restrict__ src, const WinChunk chunk,
                                                     void* scratch, Layout L, int Hs, int Ws) {
  const int v = blockIdx.y, ox = threadIdx.x;
  const Win w = chunk.v[v];
  unsigned char* slot = slot_ptr(scratch, L, v);
  const Axis* a = reinterpret_cast<const Axis*>(slot + L.axes);
  const int lo = a->lo[ox], n = a->n[ox];
  unsigned char* inter = slot + L.inter;
  for (int y = blockIdx.x; y < w.h; y += gridDim.x) {
    const unsigned char* row = src + (((size_t)w.src * Hs + (w.y0 + y)) * Ws + (w.x0 + lo)) * 3;
    int acc = 1 << (kBits - 1);
    for (int j = 0; j < n; ++j) {
      const int l = (19595 * row[3 * j] + 38470 * row[3 * j + 1] + 7471 * row[3 * j + 2] + 0x8000) >> 16;
      acc += a->k[j][ox] * l;
    }
    inter[(size_t)y * kN + ox] = (unsigned char)clip8(acc);
  }
}

__global__ __launch_bounds__(256) void gray_v_kernel(void* scratch, Layout L, unsigned char* __restrict__ gray_out) {
  const int v = blockIdx.y, oy = blockIdx.x, ox = threadIdx.x;
  unsigned char* slot = slot_ptr(scratch, L, v);
  const Axis* a = reinterpret_cast<const Axis*>(slot + L.axes) + 1;
  const unsigned char* inter = slot + L.inter;
  const int lo = a->lo[oy], n = a->n[oy];
  int acc = 1 << (kBits - 1);
  for (int j = 0; j < n; ++j) acc += a->k[j][oy] * (int)inter[(size_t)(lo + j) * kN + ox];
  const unsigned char g = (unsigned char)clip8(acc);
  slot[L.gray + oy * kN + ox] = g;
  if (gray_out) gray_out[((size_t)v * kN + oy) * kN + ox] = g;
}

// ---- exact-integer statistics ------------------------------------------------------------------------------------
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One thread = one 4 x 4 tile (a level-2 Haar cell) and its one-pixel ring.  The 5 x 5 SRM kernel is the 3 x 3 second
// derivative inside a ring of zeros, so with its padding of 2 it gives the responses of the 3 x 3 one: computed once.
__global__ __launch_bounds__(256) void stats_kernel(void* scratch, Layout L) {
  const int v = blockIdx.y, tile = blockIdx.x * 256 + threadIdx.x, ty = tile >> 6, tx = tile & 63;
  unsigned char* slot = slot_ptr(scratch, L, v);
  const unsigned char* g = slot + L.gray;
  int p[6][6];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int y = 4 * ty - 1 + r, x = 4 * tx - 1 + c;
      p[r][c] = (y >= 0 && y < kN && x >= 0 && x < kN) ? (int)g[y * kN + x] : 0;     // zero padding
    }
  long long s[kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) s[i] = 0;
  int a1[2][2];
#pragma unroll
  for (int by = 0; by < 2; ++by)
#pragma unroll
    for (int bx = 0; bx < 2; ++bx) {
      const int a = p[1 + 2 * by][1 + 2 * bx], b = p[1 + 2 * by][2 + 2 * bx], c = p[2 + 2 * by][1 + 2 * bx],
                d = p[2 + 2 * by][2 + 2 * bx];
      const int cA = a + b + c + d, cH = a + b - c - d, cV = a - b + c - d, cD = a - b - c + d;    // x 510
      a1[by][bx] = cA;
      s[0] += cA * cA, s[1] += cH * cH, s[2] += cV * cV, s[3] += cD * cD;
    }
  {
    const int a = a1[0][0], b = a1[0][1], c = a1[1][0], d = a1[1][1];
    const long long cA = a + b + c + d, cH = a + b - c - d, cV = a - b + c - d, cD = a - b - c + d;   // x 1020
    s[4] = cA * cA, s[5] = cH * cH, s[6] = cV * cV, s[7] = cD * cD;
  }
#pragma unroll
  for (int r = 1; r < 5; ++r)
#pragma unroll
    for (int c = 1; c < 5; ++c) {
      const long long n0 = -p[r - 1][c - 1] + 2 * p[r - 1][c] - p[r - 1][c + 1] + 2 * p[r][c - 1] - 4 * p[r][c] +
                           2 * p[r][c + 1] - p[r + 1][c - 1] + 2 * p[r + 1][c] - p[r + 1][c + 1];        // x 255 * 16
      const long long n1 = 4 * p[r][c] - p[r - 1][c] - p[r + 1][c] - p[r][c - 1] - p[r][c + 1];          // x 255 * 8
      s[8] += n0, s[9] += n0 * n0, s[10] += n0 * n0 * n0, s[11] += n0 * n0 * n0 * n0;
      s[12] += n1, s[13] += n1 * n1, s[14] += n1 * n1 * n1, s[15] += n1 * n1 * n1 * n1;
    }
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(slot + L.sums);
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    const long long t = wave_sum_i64(s[i]);
    if (lane_id() == 0) atomicAdd(dst + i, (unsigned long long)t);               // two's complement: signed sums add up
  }
}

// ---- FFT ---------------------------------------------------------------------------------------------------------
// 256-point Stockham radix-2 transform of the wave's own line buf[0] -> buf[0] (8 passes, ping-pong with buf[1]); lane l
// does butterflies l and l + 64 of each pass.  tw[m] = exp(-2 pi i m / 256).
__device__ __forceinline__ void fft256(double2 (*buf)[kN], const double2* tw) {
  const int l = lane_id();
  int cur = 0;
#pragma unroll
  for (int ns = 1; ns < kN; ns <<= 1) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = l + 64 * h, k = j & (ns - 1);
      const double2 w = tw[k * (128 / ns)];
      const double2 a = buf[cur][j], b = buf[cur][j + 128];
      const double2 bw = make_double2(b.x * w.x - b.y * w.y, b.x * w.y + b.y * w.x);
      const int j0 = ((j - k) << 1) + k;
      buf[cur ^ 1][j0] = make_double2(a.x + bw.x, a.y + bw.y);
      buf[cur ^ 1][j0 + ns] = make_double2(a.x - bw.x, a.y - bw.y);
    }
    cur ^= 1;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void fft_rows_kernel(void* scratch, Layout L) {
  __shared__ double2 buf[4][2][kN];
  __shared__ double2 tw[128];
  const int v = blockIdx.y, wv = wave_id(), l = lane_id(), row = blockIdx.x * 4 + wv;
  unsigned char* slot = slot_ptr(scratch, L, v);
  if (threadIdx.x < 128) tw[threadIdx.x] = reinterpret_cast<const double2*>(scratch)[threadIdx.x];
  const unsigned char* g = slot + L.gray + row * kN;
#pragma unroll
  for (int i = 0; i < 4; ++i) buf[wv][0][l + 64 * i] = make_double2((double)g[l + 64 * i] / 255.0, 0.0);
  __syncthreads();
  fft256(buf[wv], tw);
  double2* spec = reinterpret_cast<double2*>(slot + L.spec) + (size_t)row * kN;
#pragma unroll
  for (int i = 0; i < 4; ++i) spec[l + 64 * i] = buf[wv][0][l + 64 * i];
}

// geom: the three (256, 256) byte tables over the fftshift-ed plane: band 0..2, bucket 0..38, sector 0..7; 255 = none
__global__ __launch_bounds__(256) void fft_cols_kernel(void* scratch, Layout L, const unsigned char* __restrict__ geom) {
  __shared__ double2 buf[4][2][kN];
  __shared__ double2 tw[128];
  __shared__ float red[4][kCats];
  __shared__ int hist[kBins];
  const int v = blockIdx.y, t = threadIdx.x, wv = wave_id(), l = lane_id(), c0 = blockIdx.x * 4;
  unsigned char* slot = slot_ptr(scratch, L, v);
  if (t < 128) tw[t] = reinterpret_cast<const double2*>(scratch)[t];
  if (t < kBins) hist[t] = 0;
  const double2* spec = reinterpret_cast<const double2*>(slot + L.spec);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (t >> 2) + 64 * i;
    buf[t & 3][0][j] = spec[(size_t)j * kN + c0 + (t & 3)];
  }
  __syncthreads();
  fft256(buf[wv], tw);

  float acc[kCats];
#pragma unroll
  for (int i = 0; i < kCats; ++i) acc[i] = 0.f;
  const int sx = (c0 + wv + 128) & 255;
  const float pi = 3.14159265358979323846f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ky = l + 64 * i, at = (((ky + 128) & 255) << 8) + sx;
    const float2 f = make_float2((float)buf[wv][0][ky].x, (float)buf[wv][0][ky].y);   // each bin's own rounding
    const float mag = sqrtf(f.x * f.x + f.y * f.y), lg = logf(mag + 1e-6f), ph = atan2f(f.y, f.x);
    const int band = geom[at], bucket = geom[65536 + at], sector = geom[131072 + at];
#pragma unroll
    for (int b = 0; b < 3; ++b) acc[b] += band == b ? mag : 0.f;
#pragma unroll
    for (int b = 0; b < kBuckets; ++b) acc[3 + b] += bucket == b ? lg : 0.f;
#pragma unroll
    for (int b = 0; b < kSectors; ++b) acc[3 + kBuckets + b] += sector == b ? mag : 0.f;
    int bin = (int)((ph + pi) * (float)kBins / (pi + pi));                       // histc: the maximum joins the last bin
    bin = bin < 0 ? 0 : (bin > kBins - 1 ? kBins - 1 : bin);
    atomicAdd(&hist[bin], 1);
  }
#pragma unroll
  for (int i = 0; i < kCats; ++i) {
    const float s = wave_sum(acc[i]);                    // xor tree: the same order on every call
    if (l == 0) red[wv][i] = s;
  }
  __syncthreads();
  if (t < kCats)
    reinterpret_cast<float*>(slot + L.part)[blockIdx.x * kCats + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (t < kBins && hist[t]) atomicAdd(reinterpret_cast<int*>(slot + L.hist) + t, hist[t]);
}

// ---- the 24 values -----------------------------------------------------------------------------------------------
__device__ __forceinline__ double i128_to_double(__int128 v) {
  const bool neg = v < 0;
  const unsigned __int128 u = neg ? -(unsigned __int128)v : (unsigned __int128)v;
  const double d = (double)(unsigned long long)(u >> 64) * 18446744073709551616.0 + (double)(unsigned long long)u;
  return neg ? -d : d;
}

__global__ __launch_bounds__(64) void finalize_kernel(void* scratch, Layout L, float* __restrict__ out, int standardize) {
  __shared__ double tot[kCats];
  const int v = blockIdx.x, t = threadIdx.x;
  unsigned char* slot = slot_ptr(scratch, L, v);
  const int* cnt = reinterpret_cast<const int*>(reinterpret_cast<const unsigned char*>(scratch) + kCountsAt);
  if (t < kCats) {
    const float* part = reinterpret_cast<const float*>(slot + L.part);
    double s = 0.0;
    for (int b = 0; b < kColBlocks; ++b) s += (double)part[b * kCats + t];       // block order: fixed
    tot[t] = s;
  }
  __syncthreads();
  if (t != 0) return;

  double f[24];
  const double El = tot[0], Em = tot[1], Eh = tot[2], Et = ((El + Em) + Eh) + 1e-6;
  f[0] = El / Et, f[1] = Em / Et, f[2] = Eh / Et, f[3] = (Eh + 1e-6) / (El + 1e-6);
  double slope = 0.0;                                    // least squares over x = 0..38: sum (x - 19) y / 4940
  for (int b = 0; b < kBuckets; ++b) slope += (b - 19.0) * (cnt[b] ? tot[3 + b] / cnt[b] : 0.0);
  f[4] = slope / 4940.0;
  double sm[kSectors], mean = 0.0, var = 0.0;
  for (int s = 0; s < kSectors; ++s) {
    sm[s] = cnt[kBuckets + s] ? tot[3 + kBuckets + s] / cnt[kBuckets + s] : 0.0;
    mean += sm[s];
  }
  mean /= kSectors;
  for (int s = 0; s < kSectors; ++s) var += (sm[s] - mean) * (sm[s] - mean);
  f[5] = var / kSectors;
  {                                                      // the app's fp32 formula on the integer counts
    const int* hist = reinterpret_cast<const int*>(slot + L.hist);
    float total = 0.f, ent = 0.f;
    for (int b = 0; b < kBins; ++b) total += (float)hist[b];
    total += 1e-6f;
    for (int b = 0; b < kBins; ++b) {
      const float p = (float)hist[b] / total;
      ent += p * logf(p + 1e-6f);
    }
    f[6] = -(double)ent;
  }
  const long long* s = reinterpret_cast<const long long*>(slot + L.sums);
  for (int i = 0; i < 4; ++i) {
    f[7 + i] = (double)s[i] / (16384.0 * 510.0 * 510.0);
    f[11 + i] = (double)s[4 + i] / (4096.0 * 1020.0 * 1020.0);
  }
  const float abs_sum[2] = {16.f, 8.f};
  for (int k = 0; k < 2; ++k) {                          // central moments in exact 128-bit integers, then double
    const __int128 M = kN * kN, s1 = s[8 + 4 * k], s2 = s[9 + 4 * k], s3 = s[10 + 4 * k], s4 = s[11 + 4 * k];
    const __int128 c2 = M * s2 - s1 * s1;
    const __int128 c4 = M * M * M * s4 - 4 * M * M * s1 * s3 + 6 * M * s1 * s1 * s2 - 3 * s1 * s1 * s1 * s1;
    const double scale = 1.0 / (255.0 * ((double)abs_sum[k] + 1e-6));
    const double m = scale * ((double)(long long)s1 / 65536.0);
    const double va = scale * scale * (i128_to_double(c2) / 4294967296.0);
    const double m4 = scale * scale * scale * scale * (i128_to_double(c4) / 18446744073709551616.0);
    const double kurt = m4 / ((va + 1e-6) * (va + 1e-6));
    if (k == 0) f[15] = f[18] = m, f[16] = f[19] = va, f[17] = f[20] = kurt;
    else f[21] = m, f[22] = va, f[23] = kurt;
  }
  float* o = out + (size_t)v * 24;
  if (!standardize) {
    for (int i = 0; i < 24; ++i) o[i] = (float)f[i];
    return;
  }
  double mu = 0.0, sq = 0.0;                             // the app standardises the fp32 vector; unbiased std
  for (int i = 0; i < 24; ++i) f[i] = (double)(float)f[i], mu += f[i];
  mu /= 24.0;
  for (int i = 0; i < 24; ++i) sq += (f[i] - mu) * (f[i] - mu);
  const double sd = sqrt(sq / 23.0);
  for (int i = 0; i < 24; ++i) o[i] = sd < 1e-6 ? 0.f : (float)((f[i] - mu) / (sd + 1e-6));
}

}  // namespace freq
}  // namespace sgl

extern "C" {

size_t sgl_op_freq_features_scratch_bytes(int V, int Hs, int Ws) {
  if (V <= 0 || Hs <= 0 || Ws <= 0) return 0;
  return sgl::freq::layout(V < sgl::freq::kChunk ? V : sgl::freq::kChunk, Hs).total;
}

int sgl_op_freq_features(const void* src_u8_nhwc, int B, int Hs, int Ws, const sgl_view* views, int V,
                         const unsigned char* geometry, float* out, int standardize, unsigned char* gray_out,
                         void* scratch, size_t scratch_bytes, sgl_stream stream) {
  using namespace sgl::freq;
  if (!src_u8_nhwc || !views || !geometry || !out) return SGL_ERR_NULL;
  if (B <= 0 || Hs <= 0 || Ws <= 0 || V <= 0) return SGL_ERR_BAD_SHAPE;
  for (int v = 0; v < V; ++v)
    if (!sgl::view_box_ok(views[v], B, Hs, Ws)) return SGL_ERR_BAD_SHAPE;
  for (int v = 0; v < V; ++v) {
    const sgl_view& r = views[v];
    if (r.turns != 0 || r.keep_canvas != 0 || r.flip != 0) return SGL_ERR_UNSUPPORTED;
    if (r.x1 - r.x0 > kMaxSide || r.y1 - r.y0 > kMaxSide) return SGL_ERR_UNSUPPORTED;
  }
  if (!scratch) return SGL_ERR_NULL;
  if (reinterpret_cast<uintptr_t>(scratch) & 15) return SGL_ERR_UNSUPPORTED;   // double2 loads and stores
  if (scratch_bytes < sgl_op_freq_features_scratch_bytes(V, Hs, Ws)) return SGL_ERR_WORKSPACE;
  static_assert(sizeof(WinChunk) <= 2048, "a chunk of records must fit the kernel arguments");
  const Layout L = layout(V < kChunk ? V : kChunk, Hs);
  hipStream_t s = (hipStream_t)stream;
  const unsigned char* src = reinterpret_cast<const unsigned char*>(src_u8_nhwc);
  for (int v0 = 0; v0 < V; v0 += kChunk) {               // seven launches per 64 views
    const int nv = V - v0 < kChunk ? V - v0 : kChunk;
    WinChunk chunk = {};
    int hmax = 1;
    for (int v = 0; v < nv; ++v) {
      const sgl_view& r = views[v0 + v];
      chunk.v[v] = Win{r.src, r.x0, r.y0, r.x1 - r.x0, r.y1 - r.y0};
      if (r.y1 - r.y0 > hmax) hmax = r.y1 - r.y0;
    }
    unsigned char* gray = gray_out ? gray_out + (size_t)v0 * kN * kN : nullptr;
    hipLaunchKernelGGL(coef_kernel, dim3(2, nv), dim3(256), 0, s, chunk, scratch, L, geometry);
    hipLaunchKernelGGL(gray_h_kernel, dim3(hmax < 1024 ? hmax : 1024, nv), dim3(256), 0, s, src, chunk, scratch, L, Hs, Ws);
    hipLaunchKernelGGL(gray_v_kernel, dim3(kN, nv), dim3(256), 0, s, scratch, L, gray);
    hipLaunchKernelGGL(stats_kernel, dim3(16, nv), dim3(256), 0, s, scratch, L);
    hipLaunchKernelGGL(fft_rows_kernel, dim3(kN / 4, nv), dim3(256), 0, s, scratch, L);
    hipLaunchKernelGGL(fft_cols_kernel, dim3(kColBlocks, nv), dim3(256), 0, s, scratch, L, geometry);
    hipLaunchKernelGGL(finalize_kernel, dim3(nv), dim3(64), 0, s, scratch, L, out + (size_t)v0 * 24, standardize);
  }
  return hipGetLastError() == hipSuccess ? SGL_OK : SGL_ERR_HIP;
}

}  // extern "C"
