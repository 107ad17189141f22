// Gram stage of the block Jacobi step (block.hip): for the P block pairs
// (bi, bj) of a step, X = [A_bi A_bj] (m x 2W),
//     gram  : C = A_bi^T A_bj (cross) or G = X^T X (full), MFMA, split over
//             rows into partial slabs (deterministic, no float atomics);
#pragma once
#include "common.hpp"

namespace svdj {

constexpr int kGramThreads = 256;

// ------------------------------------------------------------------- gram
// MODE: GRAM_CROSS  C = A_bi^T A_bj (W x W slab per pair and row chunk);
//       GRAM_FULL   G = [A_bi A_bj]^T [..] (2W x 2W slab), one launch;
//       GRAM_SPLIT  the same 2W x 2W slab in three regions (A_bi^T A_bi,
//                   A_bj^T A_bj, A_bi^T A_bj), one per blockIdx.z: the
//                   one-launch form keeps 2W(2W+1)/2 tile accumulators, which
//                   for fp64 W = 64 exceed the register file.
// (The cross Grams of a quad step: gram_quad_kernel.)
// For fp64 W = 64 the cross products are also split over blockIdx.z in XS = 2
// row halves (x tiles), so accumulators plus the double-buffered loads fit in
// registers without spilling.
enum { GRAM_CROSS = 0, GRAM_FULL = 1, GRAM_SPLIT = 2 };

// (bi, bj) of Gram slab `pair`.
__device__ __forceinline__ void gram_pair(const int32_t* __restrict__ pairs, int pair, int& pi,
                                          int& pj) {
  pi = pairs[2 * pair];
  pj = pairs[2 * pair + 1];
}
template <typename T, int W>
__host__ __device__ constexpr int gram_xsplit() { return (sizeof(T) == 8 && W == 64) ? 2 : 1; }

// Rows per lane per slab of the fp32 W=64 cross Gram (16 = 64 bytes).  8 or
// 4 cut registers (208 -> 172) but measured slower end to end (16384^2 1 GPU
// 5.76 -> 6.08 s, 8-GPU rank plan 63.8 -> 73 ms; round 2).
constexpr int kGramLpl64 = 16;
// NV consecutive elements of one column with 16-byte vector loads.
template <typename T, int NV>
__device__ __forceinline__ void load_col16B(const T* __restrict__ p, T (&v)[NV]) {
  constexpr int PER = 16 / (int)sizeof(T);
  static_assert(NV % PER == 0, "whole 16-byte vectors");
  const f32x4* q = reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int i = 0; i < NV / PER; ++i) {
    f32x4 x = q[i];
    const T* xs = reinterpret_cast<const T*>(&x);
#pragma unroll
    for (int j = 0; j < PER; ++j) v[i * PER + j] = xs[j];
  }
}

template <typename T, int W, int MODE>
__global__ __launch_bounds__(kGramThreads) void gram_kernel(
    const T* __restrict__ A, int lda, int m_pad, const int32_t* __restrict__ pairs,
    int rows_per_chunk, T* __restrict__ slabs) {
  using M = Mfma<T>;
  constexpr bool FULL = MODE == GRAM_FULL;
  constexpr int TL = M::TILE;
  constexpr int HT = W / TL;                             // column tiles per block
  constexpr int XS = FULL ? 1 : gram_xsplit<T, W>();     // row halves over blockIdx.z
  constexpr int HTX = HT / XS;                           // x tiles of this workgroup
  constexpr int NCT = FULL ? 2 * HT : HTX + HT;          // column tiles loaded
  constexpr int NTP = FULL ? NCT * (NCT + 1) / 2 : HTX * HT;
  // rows per lane per slab: 64 bytes
  constexpr int LPL = (sizeof(T) == 4 && W == 64 && !FULL) ? kGramLpl64 : M::LPL;
  constexpr int SR = M::KG * LPL;  // rows per wave per slab
  constexpr int SLAB = FULL ? 4 * W * W : HTX * TL * W;  // this workgroup's reduction
  constexpr int WAVES = kGramThreads / SVDJ_WAVE;
  static_assert(HT % XS == 0, "x tiles split evenly");

  const int pair = blockIdx.x, chunk = blockIdx.y, nchunk = gridDim.y;
  const int region = MODE == GRAM_SPLIT ? (int)blockIdx.z / XS : 2;
  const int xpart = FULL ? 0 : (int)blockIdx.z % XS;
  int pi, pj;
  gram_pair(pairs, pair, pi, pj);
  const int bi = region == 1 ? pj : pi, bj = region == 0 ? pi : pj;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r_begin = chunk * rows_per_chunk;
  const int r_end = min(m_pad, r_begin + rows_per_chunk);

  // tile-pair list (compile-time)
  typename M::acc_t acc[NTP];
#pragma unroll
  for (int i = 0; i < NTP; ++i) acc[i] = M::zero();

  const T* colp[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    int blk, tile;
    if constexpr (FULL) {
      blk = ct < HT ? bi : bj;
      tile = ct % HT;
    } else {
      blk = ct < HTX ? bi : bj;
      tile = ct < HTX ? xpart * HTX + ct : ct - HTX;
    }
    const int col = blk * W + tile * TL + M::lane_col(lane);
    colp[ct] = A + (size_t)col * lda + M::lane_kg(lane) * LPL;
  }

  // Software pipeline: the next 32-row slab's loads are issued before this
  // slab's MFMAs, so HBM latency overlaps matrix-core work (without it the
  // kernel ran at ~2 TB/s, latency-bound, measured on MI355X at n=16384).
  int r0 = r_begin + wave * SR;
  T v[NCT][LPL];
  if (r0 < r_end) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) load_col16B<T, LPL>(colp[ct] + r0, v[ct]);
  }
  for (; r0 < r_end; r0 += WAVES * SR) {
    const int rn = r0 + WAVES * SR;
    T vn[NCT][LPL];
    if (rn < r_end) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) load_col16B<T, LPL>(colp[ct] + rn, vn[ct]);
    }
#pragma unroll
    for (int t = 0; t < LPL; ++t) {
      int idx = 0;
      if constexpr (FULL) {
#pragma unroll
        for (int a = 0; a < NCT; ++a)
#pragma unroll
          for (int b = a; b < NCT; ++b) {
            acc[idx] = M::mfma(v[a][t], v[b][t], acc[idx]);
            ++idx;
          }
      } else {
#pragma unroll
        for (int a = 0; a < HTX; ++a)
#pragma unroll
          for (int b = 0; b < HT; ++b) {
            acc[idx] = M::mfma(v[a][t], v[HTX + b][t], acc[idx]);
            ++idx;
          }
      }
    }
    if (rn < r_end) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int t = 0; t < LPL; ++t) v[ct][t] = vn[ct][t];
    }
  }

  // Combine the waves' partial tiles in LDS (sequentially, deterministic).
  __shared__ T red[SLAB];
  for (int i = threadIdx.x; i < SLAB; i += kGramThreads) red[i] = T(0);
  __syncthreads();
  for (int w = 0; w < WAVES; ++w) {
    if (wave == w) {
      int idx = 0;
      if constexpr (FULL) {
        constexpr int N = 2 * W;
#pragma unroll
        for (int a = 0; a < NCT; ++a)
#pragma unroll
          for (int b = a; b < NCT; ++b) {
#pragma unroll
            for (int e = 0; e < M::NACC; ++e) {
              const int r = a * TL + M::acc_row(e, lane);
              const int c = b * TL + M::lane_col(lane);
              red[r * N + c] += acc[idx][e];
              if (a != b) red[c * N + r] += acc[idx][e];
            }
            ++idx;
          }
      } else {
#pragma unroll
        for (int a = 0; a < HTX; ++a)
#pragma unroll
          for (int b = 0; b < HT; ++b) {
#pragma unroll
            for (int e = 0; e < M::NACC; ++e) {
              const int r = a * TL + M::acc_row(e, lane);
              const int c = b * TL + M::lane_col(lane);
              red[r * W + c] += acc[idx][e];
            }
            ++idx;
          }
      }
    }
    __syncthreads();
  }
  const int xoff = xpart * HTX * TL;  // first row of this workgroup's part
  if constexpr (MODE == GRAM_SPLIT) {  // this region's quadrant(s) of the 2W x 2W slab
    constexpr int N = 2 * W;
    T* out = slabs + ((size_t)pair * nchunk + chunk) * 4 * W * W;
    for (int i = threadIdx.x; i < SLAB; i += kGramThreads) {
      const int a = xoff + i / W, b = i % W;
      const T v = red[i];
      if (region == 0) out[a * N + b] = v;
      if (region == 1) out[(W + a) * N + W + b] = v;
      if (region == 2) {
        out[a * N + W + b] = v;
        out[(W + b) * N + a] = v;
      }
    }
  } else if constexpr (FULL) {
    T* out = slabs + ((size_t)pair * nchunk + chunk) * SLAB;
    for (int i = threadIdx.x; i < SLAB; i += kGramThreads) out[i] = red[i];
  } else {
    T* out = slabs + ((size_t)pair * nchunk + chunk) * (W * W) + xoff * W;
    for (int i = threadIdx.x; i < SLAB; i += kGramThreads) out[i] = red[i];
  }
}

// fp32 W = 64 cross Gram (GRAM_CROSS) with coalesced loads.
// gram_kernel's operand loads follow the MFMA lane map (lane = column): every
// 16-byte load instruction touches 64 columns, i.e. 64 cache lines.  Here a
// wave loads its 32-row slab of the pair's 128 columns with lanes along the
// rows (8 lanes x 16 B = one 128-byte column segment, 8 columns per
// instruction), keeps the next slab in flight in registers, and transposes
// through a wave-private LDS image [column][32 rows + 4 pad] (144-byte
// stride: conflict-free ds_read_b128 of 4 rows of a column per lane).  The
// MFMAs and the reduction are gram_kernel's; no barrier inside the row loop.
constexpr int kGlStride = 36;  // floats per column in the LDS image
template <int MODE>
__global__ __launch_bounds__(kGramThreads) void gram_cross_f32_kernel(
    const float* __restrict__ A, int lda, int m_pad, const int32_t* __restrict__ pairs,
    int rows_per_chunk, float* __restrict__ slabs, int rev) {
  static_assert(MODE == GRAM_CROSS, "cross Grams only");
  constexpr int W = 64, SR = 32, WAVES = kGramThreads / SVDJ_WAVE;
  using M = Mfma<float>;
  __shared__ float img[WAVES][2 * W * kGlStride];  // 4 x 18 KB; reused for the reduction
  // rev: row chunks dispatched last-first (the most recently written rows
  // of the previous apply first, while they may still sit in the Infinity Cache)
  const int pair = blockIdx.x, nchunk = gridDim.y,
            chunk = rev ? nchunk - 1 - (int)blockIdx.y : (int)blockIdx.y;
  int pi, pj;
  gram_pair(pairs, pair, pi, pj);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r_begin = chunk * rows_per_chunk;
  const int r_end = min(m_pad, r_begin + rows_per_chunk);
  // loads: instruction j covers columns 8j .. 8j+7 (lane >> 3), rows 4 (lane & 7) ..
  const int lc = lane >> 3, lr = (lane & 7) * 4;
  const float* src[2] = {A + (size_t)pi * W * lda, A + (size_t)pj * W * lda};
  float* im = img[wave];
  f32x4 ld[16];
  auto gload = [&](int r0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int col = 8 * j + lc;  // 0..127: x block then y block
      ld[j] = *reinterpret_cast<const f32x4*>(src[col >> 6] + (size_t)(col & 63) * lda + r0 + lr);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      *reinterpret_cast<f32x4*>(im + (8 * j + lc) * kGlStride + lr) = ld[j];
  };
  M::acc_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = M::zero();
  const int c = lane & 31, kg = lane >> 5;
  int r0 = r_begin + wave * SR;
  if (r0 < r_end) {
    gload(r0);
    lstore();
  }
  for (; r0 < r_end; r0 += WAVES * SR) {
    const int rn = r0 + WAVES * SR;
    if (rn < r_end) gload(rn);
    // rows kg*16 + t of column tile ct: 4 x ds_read_b128 per tile
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      f32x4 v[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        v[ct] = *reinterpret_cast<const f32x4*>(im + (ct * 32 + c) * kGlStride + kg * 16 + q4 * 4);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = M::mfma(v[a][t], v[2 + b][t], acc[a][b]);
    }
    if (rn < r_end) lstore();  // after this wave's reads of the image (in-order LDS)
  }
  // combine the waves' partial tiles (sequentially, deterministic)
  __syncthreads();
  float* red = &img[0][0];
  for (int i = threadIdx.x; i < W * W; i += kGramThreads) red[i] = 0.0f;
  __syncthreads();
  for (int w = 0; w < WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int e = 0; e < M::NACC; ++e)
            red[(a * 32 + M::acc_row(e, lane)) * W + b * 32 + c] += acc[a][b][e];
    }
    __syncthreads();
  }
  float* out = slabs + ((size_t)pair * nchunk + chunk) * (W * W);
  for (int i = threadIdx.x; i < W * W; i += kGramThreads) out[i] = red[i];
}

}  // namespace svdj
