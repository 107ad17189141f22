// Pack and finalize passes of svd_batched's "block" engine (models/batched.py).
//
// The engine solves a batch of matrices wider than the LDS-resident kernels
// take (batched.hip, batched_tall.hip: 64 columns) with the block path's own
// step kernels: the B matrices are stacked side by side as column blocks of
// one column-major array of m_pad rows and B ncols columns (matrix b's column
// j is stacked column b ncols + j), their V's likewise with n_v rows, and a
// step of svdj_block_steps_grouped whose pair list never crosses a matrix is
// B independent block-Jacobi steps in one launch.  This file holds what is
// per matrix before and after the steps:
//
//   svdj_stack_pack      batch (strided, read once) -> stacked image, squared
//                        column norms D, every matrix's metric words (its own
//                        underflow floor), identity blocks of the stacked V;
//   svdj_stack_finalize  stacked images (read once) -> sigma, U (batch, m, n)
//                        and V (batch, n, n) row-major.
//
// Both move 64 x 64 tiles through LDS, so the side that is contiguous along
// rows and the side that is contiguous along columns are both accessed in
// 256- or 512-byte runs.  One workgroup owns 64 stacked columns over all
// their rows, so a column's sum of squares is formed by one wave in a fixed
// order (that of post.hip's colnorm2_kernel): no atomics, and a matrix's
// numbers do not depend on its place in the batch.
#include "common.hpp"
#include "svdj_hip.h"
#include "svdj_stop.h"

namespace svdj {

constexpr int kStackTile = 64;      // tile edge; ncols and m_pad are multiples of it
constexpr int kStackThreads = 256;  // 4 waves: wave w owns tile columns w, w + 4, ...
constexpr int kStackIter = kStackTile * kStackTile / kStackThreads;  // 16 elements per thread

// grid (ncols / 64, batch).  A: element (b, i, j) at A[b sb + i sr + j sc].
template <typename T>
__global__ __launch_bounds__(kStackThreads) void stack_pack_kernel(
    const T* __restrict__ A, long long sb, long long sr, long long sc, int m, int n, int m_pad,
    int ncols, T* __restrict__ At, int lda, T* __restrict__ V, int n_v, int ldv,
    T* __restrict__ D) {
  __shared__ T tile[kStackTile][kStackTile + 1];  // [column][row]
  const int tid = threadIdx.x, lo = tid & 63, hi = tid >> 6;
  const int b = blockIdx.y, j0 = blockIdx.x * kStackTile;
  const T* Ab = A + (long long)b * sb;
  T* out = At + ((size_t)b * ncols + j0) * lda;
  const bool by_col = sc != 1 && sr == 1;  // column-major input: read along the rows
  double acc[kStackIter];
#pragma unroll
  for (int it = 0; it < kStackIter; ++it) acc[it] = 0.0;
  for (int i0 = 0; i0 < m_pad; i0 += kStackTile) {
    if (i0 < m) {
#pragma unroll
      for (int it = 0; it < kStackIter; ++it) {
        const int a = hi + 4 * it;
        const int i = i0 + (by_col ? lo : a), j = j0 + (by_col ? a : lo);
        const T x = (i < m && j < n) ? Ab[(long long)i * sr + (long long)j * sc] : T(0);
        tile[j - j0][i - i0] = x;
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < kStackIter; ++it) {
        const int jj = hi + 4 * it;
        const T x = tile[jj][lo];
        out[(size_t)jj * lda + i0 + lo] = x;
        acc[it] += (double)x * (double)x;
      }
      __syncthreads();
    } else {  // pad rows
#pragma unroll
      for (int it = 0; it < kStackIter; ++it) out[(size_t)(hi + 4 * it) * lda + i0 + lo] = T(0);
    }
  }
#pragma unroll
  for (int it = 0; it < kStackIter; ++it) {
    const double s = wave_sum(acc[it]);
    if (lo == 0) D[(size_t)b * ncols + j0 + hi + 4 * it] = (T)s;
  }
  if (V) {  // identity block of matrix b: stacked column b ncols + j has its one in row j
#pragma unroll 1
    for (int it = 0; it < kStackIter; ++it) {
      const int j = j0 + hi + 4 * it;
      T* col = V + ((size_t)b * ncols + j) * ldv;
      for (int i = lo; i < n_v; i += 64) col[i] = i == j ? T(1) : T(0);
    }
  }
}

// One workgroup per matrix: its metric words.  Floor (words 2..3) =
// max(fabs_, frel * the matrix's largest squared column norm), the formula of
// post.hip's norm_floor_scaled_kernel; every other word zero.
template <typename T>
__global__ __launch_bounds__(256) void stack_floor_kernel(const T* __restrict__ D, int ncols,
                                                          double fabs_, double frel,
                                                          uint32_t* __restrict__ metric) {
  __shared__ double wm[4];
  const T* d = D + (size_t)blockIdx.x * ncols;
  uint32_t* mt = metric + (size_t)blockIdx.x * SVDJ_METRIC_WORDS;
  double mx = 0.0;
  for (int i = threadIdx.x; i < ncols; i += 256) mx = fmax(mx, (double)d[i]);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = fmax(fmax(wm[0], wm[1]), fmax(wm[2], wm[3]));
    mt[0] = 0u; mt[1] = 0u;
    *reinterpret_cast<double*>(mt + 2) = fmax(fabs_, frel * mx);
    for (int w = 4; w < SVDJ_METRIC_WORDS; ++w) mt[w] = 0u;
  }
}

// grid (ncols / 64, batch, 2).  z = 0: 64 stacked columns of A -> sigma, and U
// (row-major, unscaled first, then scaled in place by the workgroup that wrote
// it, once the column norms are known); z = 1: the same columns of V -> Vout.
template <typename T>
__global__ __launch_bounds__(kStackThreads) void stack_finalize_kernel(
    const T* __restrict__ At, int lda, const T* __restrict__ V, int ldv, int m, int n, int ncols,
    T* __restrict__ U, T* __restrict__ S, T* __restrict__ Vout, int scale_u) {
  __shared__ T tile[kStackTile][kStackTile + 1];  // [column][row]
  __shared__ T inv[kStackTile];
  const int tid = threadIdx.x, lo = tid & 63, hi = tid >> 6;
  const int b = blockIdx.y, j0 = blockIdx.x * kStackTile;
  if (j0 >= n) return;  // padding columns only (uniform over the workgroup)
  const bool isv = blockIdx.z != 0;
  const T* src = isv ? V + ((size_t)b * ncols + j0) * ldv : At + ((size_t)b * ncols + j0) * lda;
  const int ld = isv ? ldv : lda, rows = isv ? n : m;
  T* dst = isv ? Vout + (size_t)b * n * n : (U ? U + (size_t)b * m * n : nullptr);
  if (isv && !Vout) return;
  double acc[kStackIter];
#pragma unroll
  for (int it = 0; it < kStackIter; ++it) acc[it] = 0.0;
  // rows [0, round_up(rows, 64)) exist in the image (m_pad, n_v: multiples of 128)
  for (int i0 = 0; i0 < rows; i0 += kStackTile) {
#pragma unroll
    for (int it = 0; it < kStackIter; ++it) {
      const int jj = hi + 4 * it;
      const T x = src[(size_t)jj * ld + i0 + lo];
      acc[it] += (double)x * (double)x;
      tile[jj][lo] = x;
    }
    if (dst) {
      __syncthreads();
#pragma unroll
      for (int it = 0; it < kStackIter; ++it) {
        const int i = i0 + hi + 4 * it, j = j0 + lo;
        if (i < rows && j < n) dst[(size_t)i * n + j] = tile[lo][hi + 4 * it];
      }
      __syncthreads();
    }
  }
  if (isv) return;
#pragma unroll
  for (int it = 0; it < kStackIter; ++it) {
    const double nrm = sqrt(wave_sum(acc[it]));
    const int jj = hi + 4 * it;
    if (lo == 0) {
      if (j0 + jj < n) S[(size_t)b * n + j0 + jj] = (T)nrm;
      // sigma == 0: the column stays as it is.  As in post.hip's finalize_kernel
      // the reciprocal is rounded to T: an fp32 sigma below 2^-128 (the driver's
      // per-matrix floor keeps such columns unrotated) overflows it to inf.
      inv[jj] = nrm > 0.0 ? (T)(1.0 / nrm) : T(1);
    }
  }
  if (!dst || !scale_u) return;
  __syncthreads();  // inv, and this workgroup's own stores to U
  const int j = j0 + lo;
  if (j < n) {
    const T f = inv[lo];
    for (int i = hi; i < m; i += 4) dst[(size_t)i * n + j] *= f;
  }
}

static int stack_check(const char* what, int dtype, int batch, int m, int n, int m_pad, int ncols,
                       int lda, const void* V, int n_v, int ldv) {
  if (dtype != 0 && dtype != 1) {
    set_error("%s: dtype %d (0 fp32, 1 fp64)", what, dtype);
    return -2;
  }
  if (batch < 0 || m < 1 || n < 1 || m < n) {
    set_error("%s: bad batch/m/n %d/%d/%d (m >= n >= 1)", what, batch, m, n);
    return -2;
  }
  if (m_pad < m || m_pad % SVDJ_ROW_ALIGN || lda < m_pad || ncols < n || ncols % kStackTile) {
    set_error("%s: bad m_pad/lda/ncols %d/%d/%d for m, n = %d, %d (m_pad a multiple of %d, ncols "
              "of %d)", what, m_pad, lda, ncols, m, n, SVDJ_ROW_ALIGN, kStackTile);
    return -2;
  }
  if (V && (n_v < ncols || n_v % SVDJ_ROW_ALIGN || ldv < n_v)) {
    set_error("%s: bad n_v/ldv %d/%d for ncols %d", what, n_v, ldv, ncols);
    return -2;
  }
  if ((long long)batch * ncols > 0x7fffffffLL || batch > 65535) {
    set_error("%s: %d matrices of %d stacked columns exceed the kernels' index range "
              "(65535 matrices, 2^31 - 1 columns per call)", what, batch, ncols);
    return -2;
  }
  return 0;
}

}  // namespace svdj

using namespace svdj;

extern "C" int svdj_stack_pack(int dtype, int batch, int m, int n, const void* A, long sb, long sr,
                               long sc, int m_pad, int ncols, void* At, int lda, void* V, int n_v,
                               int ldv, void* D, uint32_t* metric, void* stream) {
  const int rc = stack_check("stack_pack", dtype, batch, m, n, m_pad, ncols, lda, V, n_v, ldv);
  if (rc) return rc;
  if (batch == 0) return 0;
  if (!A || !At || !D || !metric) {
    set_error("stack_pack: null A, At, D or metric");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ncols / kStackTile, batch);
  const double tiny = dtype == 1 ? 2.2250738585072014e-308 : 1.1754943508222875e-38;
  const double fabs_ = (double)m_pad * tiny, frel = svdj_norm_floor_value(dtype, m_pad);
  if (dtype == 1) {
    hipLaunchKernelGGL(stack_pack_kernel<double>, grid, dim3(kStackThreads), 0, st,
                       (const double*)A, (long long)sb, (long long)sr, (long long)sc, m, n, m_pad,
                       ncols, (double*)At, lda, (double*)V, n_v, ldv, (double*)D);
    SVDJ_LAUNCH_CHECK();
    hipLaunchKernelGGL(stack_floor_kernel<double>, dim3(batch), dim3(256), 0, st,
                       (const double*)D, ncols, fabs_, frel, metric);
  } else {
    hipLaunchKernelGGL(stack_pack_kernel<float>, grid, dim3(kStackThreads), 0, st, (const float*)A,
                       (long long)sb, (long long)sr, (long long)sc, m, n, m_pad, ncols, (float*)At,
                       lda, (float*)V, n_v, ldv, (float*)D);
    SVDJ_LAUNCH_CHECK();
    hipLaunchKernelGGL(stack_floor_kernel<float>, dim3(batch), dim3(256), 0, st, (const float*)D,
                       ncols, fabs_, frel, metric);
  }
  SVDJ_LAUNCH_CHECK();
  return 0;
}

extern "C" int svdj_stack_finalize(int dtype, int batch, int m, int n, int m_pad, int ncols,
                                   const void* At, int lda, const void* V, int n_v, int ldv,
                                   void* U, void* S, void* Vout, int scale_u, void* stream) {
  const int rc = stack_check("stack_finalize", dtype, batch, m, n, m_pad, ncols, lda, V, n_v, ldv);
  if (rc) return rc;
  if (batch == 0) return 0;
  if (!At || !S || (Vout && !V)) {
    set_error("stack_finalize: null At or S, or a V output without the stacked V");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ncols / kStackTile, batch, Vout ? 2 : 1);
  if (dtype == 1)
    hipLaunchKernelGGL(stack_finalize_kernel<double>, grid, dim3(kStackThreads), 0, st,
                       (const double*)At, lda, (const double*)V, ldv, m, n, ncols, (double*)U,
                       (double*)S, (double*)Vout, scale_u);
  else
    hipLaunchKernelGGL(stack_finalize_kernel<float>, grid, dim3(kStackThreads), 0, st,
                       (const float*)At, lda, (const float*)V, ldv, m, n, ncols, (float*)U,
                       (float*)S, (float*)Vout, scale_u);
  SVDJ_LAUNCH_CHECK();
  return 0;
}
