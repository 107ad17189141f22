// Batched one-sided Jacobi SVD of small matrices: one workgroup per matrix,
// the matrix (and V) resident in LDS from load to store.
//
// The scalar path (scalar.hip) solves one matrix with one launch per parallel
// step; for a 32 x 32 matrix that is ~sweeps x 31 launches moving a few
// kilobytes each.  Here the grid is the batch: workgroup b reads A_b once,
// runs the whole iteration in LDS and writes U_b, S_b, V_b once.
//
// Work split.  A parallel step of the round-robin ordering holds N / 2
// disjoint column pairs (N = n rounded up to even; for odd n ring position
// N - 1 is a phantom that is never read or written).  Pair slot k of a step
// belongs to lanes [8k, 8k + 8) of the workgroup, so the workgroup has
// round_up(8 N / 2, 64) threads: one wave up to n = 16, four at n = 64.  The 8
// lanes stride the rows, reduce the dot triple with three __shfl_xor steps
// inside their group (every lane of a group gets the same bits: the xor
// butterfly adds the same operands in the same tree in every lane), solve the
// rotation redundantly and rotate the two A columns and V columns in LDS.
// The pair of (step r, slot k) is the one parallel/schedule.py
// round_robin_padded lists there, computed by index arithmetic.
//
// LDS image.  Column-major, column c of A at c * lda, lda = the smallest
// value >= m with lda = 8 (mod 32) elements (V: ldv likewise from n).  The 8
// lanes of a group touch 8 consecutive elements of a column; a 32-lane LDS
// access group holds 4 pair groups, whose columns are consecutive ring
// positions (r + k and r - k for k = 4j .. 4j + 3).  With lda = 8 (mod 32)
// consecutive columns start 8 elements apart modulo the 32 fp32 banks (16 of
// the 64 dword banks for fp64), so the 4 groups cover all banks once instead
// of piling onto the same 8.  The transposed accesses of the load and the
// store conflict at this lda; they touch every element once per solve, the
// steps ~3 (n - 1) times per sweep.
//
// Scaling.  At load the matrix is multiplied by the power of two that brings
// its largest entry into [1, 2) (exact), and sigma is scaled back at the
// store: 1e-20 A and 2^40 A iterate as A does, and squared norms of fp32 data
// never reach the subnormal range.  The underflow floor of the block path
// (svdj_set_norm_floor_scaled) is then taken from the largest squared column
// norm of the scaled matrix.
//
// Barriers: one __syncthreads per step, reached by every thread (idle groups,
// phantom and skipped pairs and converged or non-finite matrices fall
// through to it); the sweep loop is counted and its break is uniform.
#include "batched_core.hpp"
#include "svdj_hip.h"

namespace svdj {

// The one LDS layout: the size routine and the kernel both use it.
struct BatchedLayout {
  long lda, ldv;
  size_t a_off, v_off, sig_off, scr_off, bytes;
};
__host__ __device__ inline BatchedLayout batched_layout(int esize, int m, int n, int want_v) {
  BatchedLayout L;
  L.lda = batched_ld(m);
  L.ldv = want_v ? batched_ld(n) : 0;
  L.a_off = 0;
  L.v_off = (size_t)L.lda * n * esize;
  L.sig_off = L.v_off + (size_t)L.ldv * n * esize;
  L.scr_off = L.sig_off + (size_t)kBatchedMaxN * esize;
  L.bytes = L.scr_off + kBatchedScratch;
  return L;
}

__host__ __device__ constexpr int batched_threads(int n) {
  return round_up((n + (n & 1)) / 2 * kBatchedLanes, SVDJ_WAVE);
}

// The iteration itself (floor, sweeps, stop test, finalize) is batched_core.hpp.
template <typename T>
__global__ __launch_bounds__(kBatchedMaxThreads) void batched_svd_kernel(
    int m, int n, const T* __restrict__ A, long sb, long sr, long sc, T* __restrict__ U,
    T* __restrict__ S, T* __restrict__ V, double tol_in, int tol_mode, int max_sweeps,
    int32_t* __restrict__ sweeps_out, float* __restrict__ off_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool want_v = V != nullptr;
  const BatchedLayout L = batched_layout((int)sizeof(T), m, n, want_v ? 1 : 0);
  T* As = reinterpret_cast<T*>(smem + L.a_off);
  T* Vs = reinterpret_cast<T*>(smem + L.v_off);
  T* sig = reinterpret_cast<T*>(smem + L.sig_off);
  BatchedScratch* scr = reinterpret_cast<BatchedScratch*>(smem + L.scr_off);
  const int lda = (int)L.lda, ldv = (int)L.ldv;

  const BatchedThread t = batched_thread();
  const int tid = t.tid, nthr = t.nthr, nwave = t.nwave, lane = t.lane, wave = t.wave;
  const size_t b = blockIdx.x;
  const int total = m * n;

  // ---- load A_b, coalesced along whichever of row / column has unit stride
  const T* Ab = A + (long)b * sb;
  T amax = 0;
  if (sr == 1 && sc != 1) {
    for (int idx = tid; idx < total; idx += nthr) {
      const int j = idx / m, i = idx - j * m;
      const T x = Ab[(long)i * sr + (long)j * sc];
      As[j * lda + i] = x;
      amax = fmax(amax, fabs(x));
    }
  } else {
    for (int idx = tid; idx < total; idx += nthr) {
      const int i = idx / n, j = idx - i * n;
      const T x = Ab[(long)i * sr + (long)j * sc];
      As[j * lda + i] = x;
      amax = fmax(amax, fabs(x));
    }
  }
  if (want_v)
    for (int idx = tid; idx < n * n; idx += nthr) {
      const int j = idx / n, i = idx - j * n;
      Vs[j * ldv + i] = (i == j) ? T(1) : T(0);
    }
  amax = wave_max(amax);
  if (lane == 0) scr->red[0][wave] = (double)amax;
  __syncthreads();
  double am = 0.0;
  for (int w = 0; w < nwave; ++w) am = fmax(am, scr->red[0][w]);
  // power-of-two scale: largest entry into [1, 2); 0 and non-finite: none
  int ex = 0;
  if (am > 0.0 && am <= (double)std::numeric_limits<T>::max()) ex = ilogb(am);

  // ---- scale, squared column norms, floor; sweeps; sigma and U
  const T floor_ = batched_scale_floor(As, lda, m, n, ex, scr, t);
  const T tol = batched_scaled_tol<T>(tol_in, tol_mode, ex);
  int sweeps;
  float last_off;
  batched_sweeps(As, lda, Vs, ldv, m, n, want_v, tol, tol_mode, floor_, max_sweeps, scr, t,
                 sweeps, last_off);
  batched_finalize(As, lda, m, n, ex, sig, U != nullptr, t);
  __syncthreads();

  // ---- store: row-major outputs, consecutive lanes on consecutive columns
  if (tid < n) S[b * n + tid] = sig[tid];
  if (U != nullptr) {
    T* Ub = U + b * (size_t)total;
    for (int idx = tid; idx < total; idx += nthr) {
      const int i = idx / n, j = idx - i * n;
      Ub[idx] = As[j * lda + i];
    }
  }
  if (want_v) {
    T* Vb = V + b * (size_t)n * n;
    for (int idx = tid; idx < n * n; idx += nthr) {
      const int i = idx / n, j = idx - i * n;
      Vb[idx] = Vs[j * ldv + i];
    }
  }
  if (tid == 0) {
    sweeps_out[b] = sweeps;
    off_out[b] = last_off;
  }
}

template <typename T>
static int batched_launch(int batch, int m, int n, const void* A, long sb, long sr, long sc,
                          void* U, void* S, void* V, double tol, int tol_mode, int max_sweeps,
                          int32_t* sweeps, float* off, size_t lds, hipStream_t st) {
  if (lds > 65536) {  // above 64 KiB dynamic LDS is an opt-in per kernel
    SVDJ_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&batched_svd_kernel<T>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kBatchedLdsCap));
  }
  hipLaunchKernelGGL(batched_svd_kernel<T>, dim3(batch), dim3(batched_threads(n)), lds, st, m, n,
                     (const T*)A, sb, sr, sc, (T*)U, (T*)S, (T*)V, tol, tol_mode, max_sweeps,
                     sweeps, off);
  SVDJ_LAUNCH_CHECK();
  return 0;
}

}  // namespace svdj

using namespace svdj;

extern "C" size_t svdj_batched_lds_bytes(int dtype, int m, int n, int want_v) {
  if ((dtype != 0 && dtype != 1) || n < 1 || n > kBatchedMaxN || m < n) return 0;
  const BatchedLayout L = batched_layout(dtype == 1 ? 8 : 4, m, n, want_v ? 1 : 0);
  return L.bytes <= kBatchedLdsCap ? L.bytes : 0;
}

extern "C" int svdj_batched_threads(int n) {
  return (n < 1 || n > kBatchedMaxN) ? 0 : batched_threads(n);
}

extern "C" int svdj_batched_svd(int dtype, int batch, int m, int n, const void* A, long sb,
                                long sr, long sc, void* U, void* S, void* V, double tol,
                                int tol_mode, int max_sweeps, int32_t* sweeps, float* off,
                                void* stream) {
  if (dtype != 0 && dtype != 1) {
    set_error("batched_svd: unsupported dtype %d (0 fp32, 1 fp64)", dtype);
    return -2;
  }
  if (batch < 0 || n < 1 || m < n) {
    set_error("batched_svd: bad shape batch %d, %d x %d (needs batch >= 0, m >= n >= 1)", batch,
              m, n);
    return -2;
  }
  if (n > kBatchedMaxN) {
    set_error("batched_svd: n = %d columns, at most %d", n, kBatchedMaxN);
    return -2;
  }
  const size_t lds = svdj_batched_lds_bytes(dtype, m, n, V != nullptr);
  if (lds == 0) {
    set_error("batched_svd: %d x %d (%s) does not fit in %zu bytes of LDS", m, n,
              dtype == 1 ? "fp64" : "fp32", kBatchedLdsCap);
    return -2;
  }
  if (max_sweeps < 0) {
    set_error("batched_svd: max_sweeps %d < 0", max_sweeps);
    return -2;
  }
  if (batch == 0) return 0;
  if (A == nullptr || S == nullptr || sweeps == nullptr || off == nullptr) {
    set_error("batched_svd: A, S, sweeps and off must not be NULL");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    return batched_launch<float>(batch, m, n, A, sb, sr, sc, U, S, V, tol, tol_mode, max_sweeps,
                                 sweeps, off, lds, st);
  return batched_launch<double>(batch, m, n, A, sb, sr, sc, U, S, V, tol, tol_mode, max_sweeps,
                                sweeps, off, lds, st);
}
