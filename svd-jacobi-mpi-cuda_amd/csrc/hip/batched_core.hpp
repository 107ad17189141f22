// The LDS-resident one-sided Jacobi iteration of the batched kernels, as
// __device__ functions: the floor, the sweep loop with its stop test, and the
// sigma / U finalize.  batched.hip runs them on the whole matrix,
// batched_tall.hip on the n x n factor R of its QR stage.  Every function
// here is called by all threads of the workgroup (they hold barriers).
//
// Work split, LDS image and barriers: see the header of batched.hip.
#pragma once
#include "common.hpp"

#include <limits>

namespace svdj {

constexpr int kBatchedLanes = 8;          // lanes per column pair
constexpr int kBatchedMaxN = 64;          // columns (pairs x lanes <= 256 threads)
constexpr int kBatchedMaxThreads = 256;
constexpr size_t kBatchedLdsCap = 163840;  // one workgroup may take the CU's 160 KiB
constexpr int kBatchedScratch = 128;      // sweep flags and reduction slots

// Leading dimension of an LDS image with `rows` rows: >= rows, = 8 (mod 32).
__host__ __device__ constexpr long batched_ld(long rows) {
  return rows <= 8 ? 8 : (rows - 8 + 31) / 32 * 32 + 8;
}

template <typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int o = kBatchedLanes / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, SVDJ_WAVE);
  return v;
}

struct BatchedScratch {
  float off[2][4];   // per sweep parity, per wave: largest convergence value
  int rot[2][4];     // ... : any rotation applied
  double red[2][4];  // per wave: load-time reductions ([0] amax, [1] dmax)
};
static_assert(sizeof(BatchedScratch) <= kBatchedScratch, "scratch");

// A thread's place in the workgroup: wave and lane, and 8-lane group and lane in it.
struct BatchedThread {
  int tid, nthr, nwave, lane, wave, grp, g, ngrp;
};
__device__ __forceinline__ BatchedThread batched_thread() {
  BatchedThread t;
  t.tid = threadIdx.x;
  t.nthr = blockDim.x;
  t.nwave = t.nthr >> 6;
  t.lane = t.tid & 63;
  t.wave = t.tid >> 6;
  t.grp = t.tid / kBatchedLanes;
  t.g = t.tid % kBatchedLanes;
  t.ngrp = t.nthr / kBatchedLanes;
  return t;
}

// Scale the image by 2^-ex (exact; ex = 0: as is), take the squared column
// norms and return the underflow floor of the block path
// (svdj_set_norm_floor_scaled) from the largest one.  One barrier.
template <typename T>
__device__ __forceinline__ T batched_scale_floor(T* As, int lda, int m, int n, int ex,
                                                 BatchedScratch* scr, const BatchedThread& t) {
  T dmax = 0;
  for (int j = t.grp; j < n; j += t.ngrp) {
    T* a = As + j * lda;
    T d = 0;
    for (int i = t.g; i < m; i += kBatchedLanes) {
      const T x = ex != 0 ? (T)scalbn(a[i], -ex) : a[i];
      a[i] = x;
      d += x * x;
    }
    d = group_sum(d);
    dmax = fmax(dmax, d);
  }
  dmax = wave_max(dmax);
  if (t.lane == 0) scr->red[1][t.wave] = (double)dmax;
  __syncthreads();
  double dm = 0.0;
  for (int w = 0; w < t.nwave; ++w) dm = fmax(dm, scr->red[1][w]);
  // svdj_set_norm_floor_scaled: max(m realmin, m realmin / eps * dmax)
  const double tiny = (double)std::numeric_limits<T>::min();
  const double eps = (double)std::numeric_limits<T>::epsilon();
  return (T)fmax((double)m * tiny, (double)m * tiny / eps * dm);
}

// The relative test is scale free.  The absolute one is the caller's
// |a_p.a_q| > tol on the unscaled matrix: products of the scaled columns
// are 2^(-2 ex) times the caller's, and so is the threshold (0 or inf
// where it leaves T's range: every / no nonzero product exceeds it).
template <typename T>
__device__ __forceinline__ T batched_scaled_tol(double tol_in, int tol_mode, int ex) {
  return (T)(tol_mode == 1 ? scalbn(tol_in, -2 * ex) : tol_in);
}

// Sweeps of the round-robin ordering over the m x n image As (and V) until a
// sweep rotates nothing or max_sweeps: one barrier per step.
template <typename T>
__device__ __forceinline__ void batched_sweeps(T* As, int lda, T* Vs, int ldv, int m, int n,
                                               bool want_v, T tol, int tol_mode, T floor_,
                                               int max_sweeps, BatchedScratch* scr,
                                               const BatchedThread& t, int& sweeps,
                                               float& last_off) {
  const int grp = t.grp, g = t.g;
  const int N = n + (n & 1), half = N / 2, steps = N - 1;
  sweeps = 0;
  last_off = __builtin_inff();  // no sweep run: nothing measured
  for (int sw = 0; sw < max_sweeps; ++sw) {
    int rotated = 0;
    float offmax = 0.0f;
    for (int r = 0; r < steps; ++r) {
      // pair of (step r, slot grp): round_robin_padded
      int p = -1, q = -1;
      if (grp < half) {
        if (grp == 0) {
          p = r;
          q = N - 1;
        } else {
          int a = r + grp, c = r - grp + (N - 1);
          if (a >= N - 1) a -= N - 1;
          if (c >= N - 1) c -= N - 1;
          p = a < c ? a : c;
          q = a < c ? c : a;
        }
      }
      const bool valid = p >= 0 && q < n;  // q >= n: the phantom position
      T* ap = As + (valid ? p : 0) * lda;
      T* aq = As + (valid ? q : 0) * lda;
      const int rows = valid ? m : 0;
      T alpha = 0, beta = 0, gamma = 0;
      for (int i = g; i < rows; i += kBatchedLanes) {
        const T x = ap[i], y = aq[i];
        alpha += x * y;
        beta += x * x;
        gamma += y * y;
      }
      alpha = group_sum(alpha);
      beta = group_sum(beta);
      gamma = group_sum(gamma);
      const T nrm = sqrt(beta) * sqrt(gamma);
      if (valid && nrm > T(0)) {
        const float cv = (float)(fabs(alpha) / nrm);
        offmax = cv > offmax ? cv : offmax;  // drops NaN
      }
      bool rotate = (tol_mode == 1) ? (fabs(alpha) > tol)
                                    : (nrm > T(0) && fabs(alpha) > tol * nrm);
      rotate = rotate && valid && alpha != T(0) && fmin(beta, gamma) > floor_;
      if (rotate) {
        T c, s, tt;
        schur_rotation(alpha, beta, gamma, c, s, tt);
        rotated = 1;
        for (int i = g; i < m; i += kBatchedLanes) {
          const T x = ap[i], y = aq[i];
          ap[i] = c * x - s * y;
          aq[i] = s * x + c * y;
        }
        if (want_v) {
          T* vp = Vs + p * ldv;
          T* vq = Vs + q * ldv;
          for (int i = g; i < n; i += kBatchedLanes) {
            const T x = vp[i], y = vq[i];
            vp[i] = c * x - s * y;
            vq[i] = s * x + c * y;
          }
        }
      }
      if (r == steps - 1) {  // the sweep's flags ride on its last barrier
        const int any = __any(rotated);
        const float om = wave_max(offmax);
        if (t.lane == 0) {
          scr->rot[sw & 1][t.wave] = any;
          scr->off[sw & 1][t.wave] = om;
        }
      }
      __syncthreads();
    }
    int any = 0;
    float om = 0.0f;
    for (int w = 0; w < t.nwave; ++w) {
      any |= scr->rot[sw & 1][w];
      om = fmaxf(om, scr->off[sw & 1][w]);
    }
    sweeps = sw + 1;
    last_off = om;
    if (!any) break;  // uniform: every thread read the same flags
  }
}

// sigma_j = 2^ex ||a_j|| (fp64 sum) into sig; with scale_u, a_j /= ||a_j||
// (a zero column: as is).  No barrier: the caller sets one before it reads.
template <typename T>
__device__ __forceinline__ void batched_finalize(T* As, int lda, int m, int n, int ex, T* sig,
                                                 bool scale_u, const BatchedThread& t) {
  for (int j = t.grp; j < n; j += t.ngrp) {
    T* a = As + j * lda;
    double acc = 0.0;
    for (int i = t.g; i < m; i += kBatchedLanes) {
      const double x = (double)a[i];
      acc += x * x;
    }
    acc = group_sum(acc);
    const double nrm = sqrt(acc);
    if (t.g == 0) sig[j] = (T)scalbn(nrm, ex);
    if (scale_u && nrm > 0.0) {
      const T inv = (T)(1.0 / nrm);
      for (int i = t.g; i < m; i += kBatchedLanes) a[i] *= inv;
    }
  }
}

}  // namespace svdj
