// Batched SVD of tall matrices of any row count (n <= 64 columns): one
// workgroup of 256 threads per matrix, a flat-tree TSQR in front of the
// LDS-resident Jacobi of batched.hip.
//
// Phase 1, QR.  The workgroup streams A_b through LDS in panels of P rows and
// folds each panel into a resident n x n upper triangle R (zero at the
// start) with n Householder reflectors: reflector j is formed from
// (R[j][j], panel[:, j]) by LAPACK's larfg convention (beta = -sign(alpha)
// norm, sign(0) = +, tau = 0 where the panel part is exactly zero) and
// applied to the columns c > j of [R; panel]: LAPACK's xTPQRT2 with l = 0.
// An 8-lane group owns column c = j + 1 + group (and c + 32): in one pass it
// reads panel[:, j] and its columns, accumulates x.x and x.y together,
// reduces with group_sum, forms beta and tau (every group the same bits: same
// operands, same tree) and updates its columns.  Column j stays raw in
// place; 1 / (alpha - beta), tau and beta go to per-reflector LDS slots, and
// the scaling v = x / (alpha - beta) is applied when the panel is written
// out.  One barrier per reflector.  With U wanted, the panel's reflector
// vectors go to that panel's rows of the U output and the taus to tau_ws.
//
// Phase 2, Jacobi on R with V: the floor, sweep loop, stop test and finalize
// of batched_core.hpp with m = n.  The R image then holds W = U_R.
//
// Phase 3, U = Q [W; 0].  Panels from last to first: the panel's reflectors
// and taus are loaded back, a second panel image Z starts as zero, and
// H_{n-1} ... H_0 are applied to [W; Z] for all n columns.  Group `group`
// owns columns group and group + 32 of [W; Z] through all n reflectors, the
// reflectors are read only: no barrier between reflectors.  Z is stored over
// the reflectors in U.  The virtual top rows left in W at the end are the
// part of U that multiplies the zero start of R: rounding-level times the
// matrix's condition number, and dropped.  The two panel images are why the
// layout carries two of them; phase 1 uses the first only.
//
// Scaling: a running exponent.  Each panel is scaled at load by 2^-ex, ex the
// exponent of the largest entry seen so far (that panel included); when ex
// rises, R is rescaled by the exact power of two first.  c A for a power of
// two c shifts every ex by log2 c and so iterates bitwise as A does; sigma
// is scaled back at the store and the absolute tolerance as in batched.hip.
// Against a first max-abs pass over A this saves a second read of A from
// memory; it costs one block reduction and one more barrier per panel, and a
// pass over R (n^2 / 256 elements per thread) each time the exponent rises.
// Entries of early panels sit below [1, 2) when a later panel is larger; a
// rescaled R entry that drops under realmin (a matrix whose rows differ by
// more than 2^126 in fp32) is flushed, which the one-pass scaling shares.
//
// LDS images are column-major with ld = 8 (mod 32) as in batched.hip: the 4
// groups of a 32-lane access read one x (a broadcast) and 4 consecutive
// columns, which start 8 banks apart.
#include "batched_core.hpp"
#include "svdj_hip.h"

namespace svdj {

constexpr int kTallThreads = 256;
constexpr int kTallGroups = kTallThreads / kBatchedLanes;  // 32
constexpr int kTallNoExp = -(1 << 20);                     // no nonzero entry seen yet

// The one LDS layout: the size routines and the kernel both use it.
//   R image n x ldr | V image n x ldv (want_v) | panel image n x ldp |
//   Z image n x ldp | tau[64] | 1 / (alpha - beta) [64] | beta[64] |
//   sigma[64] | scratch
struct BatchedTallLayout {
  long ldr, ldv, ldp;
  size_t r_off, v_off, p_off, z_off, tau_off, scl_off, bet_off, sig_off, scr_off, bytes;
};
__host__ __device__ inline BatchedTallLayout batched_tall_layout(int esize, int n, int want_v,
                                                                 int panel_rows) {
  BatchedTallLayout L;
  L.ldr = batched_ld(n);
  L.ldv = want_v ? batched_ld(n) : 0;
  L.ldp = batched_ld(panel_rows);
  L.r_off = 0;
  L.v_off = (size_t)L.ldr * n * esize;
  L.p_off = L.v_off + (size_t)L.ldv * n * esize;
  L.z_off = L.p_off + (size_t)L.ldp * n * esize;
  L.tau_off = L.z_off + (size_t)L.ldp * n * esize;
  L.scl_off = L.tau_off + (size_t)kBatchedMaxN * esize;
  L.bet_off = L.scl_off + (size_t)kBatchedMaxN * esize;
  L.sig_off = L.bet_off + (size_t)kBatchedMaxN * esize;
  L.scr_off = L.sig_off + (size_t)kBatchedMaxN * esize;
  L.bytes = L.scr_off + kBatchedScratch;
  return L;
}

// The largest multiple of 8 whose layout fits in `limit` bytes (0: none).
static int tall_rows_within(int esize, int n, int want_v, size_t limit) {
  int p = 0;
  while (batched_tall_layout(esize, n, want_v, p + 8).bytes <= limit) p += 8;
  return p;
}

template <typename T>
__global__ __launch_bounds__(kTallThreads) void batched_tall_svd_kernel(
    int m, int n, int P, const T* __restrict__ A, long sb, long sr, long sc, T* U,
    T* __restrict__ S, T* __restrict__ V, T* tau_ws, double tol_in, int tol_mode,
    int max_sweeps, int32_t* __restrict__ sweeps_out, float* __restrict__ off_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool want_v = V != nullptr, want_u = U != nullptr;
  const BatchedTallLayout L = batched_tall_layout((int)sizeof(T), n, want_v ? 1 : 0, P);
  T* Rs = reinterpret_cast<T*>(smem + L.r_off);
  T* Vs = reinterpret_cast<T*>(smem + L.v_off);
  T* Ps = reinterpret_cast<T*>(smem + L.p_off);
  T* Zs = reinterpret_cast<T*>(smem + L.z_off);
  T* taus = reinterpret_cast<T*>(smem + L.tau_off);
  T* scl = reinterpret_cast<T*>(smem + L.scl_off);
  T* bet = reinterpret_cast<T*>(smem + L.bet_off);
  T* sig = reinterpret_cast<T*>(smem + L.sig_off);
  BatchedScratch* scr = reinterpret_cast<BatchedScratch*>(smem + L.scr_off);
  const int ldr = (int)L.ldr, ldv = (int)L.ldv, ldp = (int)L.ldp;

  const BatchedThread t = batched_thread();
  const int tid = t.tid, nthr = t.nthr, grp = t.grp, g = t.g;
  const size_t b = blockIdx.x;
  const int np = (m + P - 1) / P, cnt = P * n;
  const T* Ab = A + (long)b * sb;
  T* Ub = want_u ? U + b * (size_t)m * n : nullptr;
  T* tb = want_u ? tau_ws + b * (size_t)np * n : nullptr;
  const bool by_col = sr == 1 && sc != 1;  // element idx of a panel: (j, i) or (i, j)

  for (int idx = tid; idx < n * ldr; idx += nthr) Rs[idx] = T(0);
  if (want_v)
    for (int idx = tid; idx < n * n; idx += nthr) {
      const int j = idx / n, i = idx - j * n;
      Vs[j * ldv + i] = (i == j) ? T(1) : T(0);
    }

  // ---- phase 1: fold the panels into R
  int ex = kTallNoExp;
  for (int p = 0; p < np; ++p) {
    const int r0 = p * P, rows = min(P, m - r0);
    // load, zero padded, coalesced along whichever of row / column has unit stride
    T amax = 0;
    for (int idx = tid; idx < cnt; idx += nthr) {
      int i, j;
      if (by_col) {
        j = idx / P;
        i = idx - j * P;
      } else {
        i = idx / n;
        j = idx - i * n;
      }
      const T x = i < rows ? Ab[(long)(r0 + i) * sr + (long)j * sc] : T(0);
      Ps[j * ldp + i] = x;
      amax = fmax(amax, fabs(x));
    }
    amax = wave_max(amax);
    if (t.lane == 0) scr->red[p & 1][t.wave] = (double)amax;
    __syncthreads();
    double am = 0.0;
    for (int w = 0; w < t.nwave; ++w) am = fmax(am, scr->red[p & 1][w]);
    // running exponent: the largest entry so far into [1, 2); 0 and non-finite: none
    int down = 0;
    if (am > 0.0 && am <= (double)std::numeric_limits<T>::max()) {
      const int e = ilogb(am);
      if (e > ex) {
        down = ex == kTallNoExp ? 0 : e - ex;
        ex = e;
      }
    }
    if (down != 0)
      for (int idx = tid; idx < n * ldr; idx += nthr) Rs[idx] = (T)scalbn(Rs[idx], -down);
    if (ex != kTallNoExp && ex != 0)
      for (int idx = tid; idx < cnt; idx += nthr) {  // the elements this thread loaded
        int i, j;
        if (by_col) {
          j = idx / P;
          i = idx - j * P;
        } else {
          i = idx / n;
          j = idx - i * n;
        }
        Ps[j * ldp + i] = (T)scalbn(Ps[j * ldp + i], -ex);
      }
    __syncthreads();

    for (int j = 0; j < n; ++j) {
      const int c1 = j + 1 + grp, c2 = c1 + kTallGroups;
      const bool h1 = c1 < n, h2 = c2 < n;
      if (h1 || grp == 0) {  // group 0 also records the reflector
        const T* x = Ps + j * ldp;
        T* y1 = Ps + (h1 ? c1 : j) * ldp;
        T* y2 = Ps + (h2 ? c2 : j) * ldp;
        T xx = 0, xy1 = 0, xy2 = 0;
        for (int i = g; i < P; i += kBatchedLanes) {
          const T xv = x[i];
          xx += xv * xv;
          xy1 += xv * y1[i];
          xy2 += xv * y2[i];
        }
        xx = group_sum(xx);
        xy1 = group_sum(xy1);
        xy2 = group_sum(xy2);
        const T alpha = Rs[j * ldr + j];
        if (xx != T(0)) {
          const T nrm = sqrt(alpha * alpha + xx);
          const T beta = alpha >= T(0) ? -nrm : nrm;
          const T tau = (beta - alpha) / beta;
          const T inv = T(1) / (alpha - beta);
          if (h1) {
            const T tw = tau * (Rs[c1 * ldr + j] + inv * xy1);
            if (g == 0) Rs[c1 * ldr + j] -= tw;
            const T f = tw * inv;
            for (int i = g; i < P; i += kBatchedLanes) y1[i] -= f * x[i];
          }
          if (h2) {
            const T tw = tau * (Rs[c2 * ldr + j] + inv * xy2);
            if (g == 0) Rs[c2 * ldr + j] -= tw;
            const T f = tw * inv;
            for (int i = g; i < P; i += kBatchedLanes) y2[i] -= f * x[i];
          }
          if (tid == 0) {
            taus[j] = tau;
            scl[j] = inv;
            bet[j] = beta;  // R[j][j] itself is still read by the other groups
          }
        } else if (tid == 0) {  // H = I
          taus[j] = T(0);
          scl[j] = T(0);
          bet[j] = alpha;
        }
      }
      __syncthreads();
    }
    if (tid < n) Rs[tid * ldr + tid] = bet[tid];
    if (want_u) {
      for (int idx = tid; idx < rows * n; idx += nthr) {
        const int i = idx / n, j = idx - i * n;
        Ub[(size_t)r0 * n + idx] = Ps[j * ldp + i] * scl[j];
      }
      if (tid < n) tb[p * n + tid] = taus[tid];
    }
    __syncthreads();
  }

  // ---- phase 2: Jacobi on R (batched_core.hpp, m = n); the R image becomes W = U_R
  const int pe = ex == kTallNoExp ? 0 : ex;
  const T floor_ = batched_scale_floor(Rs, ldr, n, n, 0, scr, t);
  const T tol = batched_scaled_tol<T>(tol_in, tol_mode, pe);
  int sweeps;
  float last_off;
  batched_sweeps(Rs, ldr, Vs, ldv, n, n, want_v, tol, tol_mode, floor_, max_sweeps, scr, t,
                 sweeps, last_off);
  batched_finalize(Rs, ldr, n, n, pe, sig, want_u, t);
  __syncthreads();
  if (tid < n) S[b * n + tid] = sig[tid];
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
  if (!want_u) return;

  // ---- phase 3: U = Q [W; 0], panels from last to first
  for (int p = np - 1; p >= 0; --p) {
    const int r0 = p * P, rows = min(P, m - r0);
    // every thread reads back the elements it stored in phase 1 (same idx -> thread map)
    for (int idx = tid; idx < cnt; idx += nthr) {
      const int i = idx / n, j = idx - i * n;
      Ps[j * ldp + i] = i < rows ? Ub[(size_t)r0 * n + idx] : T(0);
      Zs[j * ldp + i] = T(0);
    }
    if (tid < n) taus[tid] = tb[p * n + tid];
    __syncthreads();
    const int c1 = grp, c2 = grp + kTallGroups;
    const bool h1 = c1 < n, h2 = c2 < n;
    if (h1) {
      T* z1 = Zs + c1 * ldp;
      T* z2 = Zs + (h2 ? c2 : c1) * ldp;
      for (int j = n - 1; j >= 0; --j) {
        const T tau = taus[j];
        if (tau == T(0)) continue;  // H = I (uniform)
        const T* x = Ps + j * ldp;
        T d1 = 0, d2 = 0;
        for (int i = g; i < P; i += kBatchedLanes) {
          const T xv = x[i];
          d1 += xv * z1[i];
          d2 += xv * z2[i];
        }
        d1 = group_sum(d1);
        d2 = group_sum(d2);
        const T tw1 = tau * (Rs[c1 * ldr + j] + d1);
        if (g == 0) Rs[c1 * ldr + j] -= tw1;
        for (int i = g; i < P; i += kBatchedLanes) z1[i] -= tw1 * x[i];
        if (h2) {
          const T tw2 = tau * (Rs[c2 * ldr + j] + d2);
          if (g == 0) Rs[c2 * ldr + j] -= tw2;
          for (int i = g; i < P; i += kBatchedLanes) z2[i] -= tw2 * x[i];
        }
      }
    }
    __syncthreads();
    for (int idx = tid; idx < rows * n; idx += nthr) {
      const int i = idx / n, j = idx - i * n;
      Ub[(size_t)r0 * n + idx] = Zs[j * ldp + i];
    }
    __syncthreads();
  }
}

template <typename T>
static int batched_tall_launch(int batch, int m, int n, int P, const void* A, long sb, long sr,
                               long sc, void* U, void* S, void* V, void* tau_ws, double tol,
                               int tol_mode, int max_sweeps, int32_t* sweeps, float* off,
                               size_t lds, hipStream_t st) {
  if (lds > 65536) {  // above 64 KiB dynamic LDS is an opt-in per kernel
    SVDJ_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&batched_tall_svd_kernel<T>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBatchedLdsCap));
  }
  hipLaunchKernelGGL(batched_tall_svd_kernel<T>, dim3(batch), dim3(kTallThreads), lds, st, m, n,
                     P, (const T*)A, sb, sr, sc, (T*)U, (T*)S, (T*)V, (T*)tau_ws, tol, tol_mode,
                     max_sweeps, sweeps, off);
  SVDJ_LAUNCH_CHECK();
  return 0;
}

}  // namespace svdj

using namespace svdj;

extern "C" size_t svdj_batched_tall_lds_bytes(int dtype, int n, int want_v, int panel_rows) {
  if ((dtype != 0 && dtype != 1) || n < 1 || n > kBatchedMaxN) return 0;
  if (panel_rows < 8 || panel_rows % 8 != 0 || panel_rows > (1 << 20)) return 0;
  const BatchedTallLayout L = batched_tall_layout(dtype == 1 ? 8 : 4, n, want_v ? 1 : 0, panel_rows);
  return L.bytes <= kBatchedLdsCap ? L.bytes : 0;
}

// Two workgroups per CU (half the LDS each) where that leaves a panel at
// least as tall as the widest R (64 rows); else the largest panel one
// workgroup can take.
extern "C" int svdj_batched_tall_panel_rows(int dtype, int n, int want_v) {
  if ((dtype != 0 && dtype != 1) || n < 1 || n > kBatchedMaxN) return 0;
  const int esize = dtype == 1 ? 8 : 4;
  const int half = tall_rows_within(esize, n, want_v ? 1 : 0, kBatchedLdsCap / 2);
  return half >= kBatchedMaxN ? half : tall_rows_within(esize, n, want_v ? 1 : 0, kBatchedLdsCap);
}

extern "C" int svdj_batched_tall_svd(int dtype, int batch, int m, int n, const void* A, long sb,
                                     long sr, long sc, void* U, void* S, void* V, void* tau_ws,
                                     int panel_rows, double tol, int tol_mode, int max_sweeps,
                                     int32_t* sweeps, float* off, void* stream) {
  if (dtype != 0 && dtype != 1) {
    set_error("batched_tall_svd: unsupported dtype %d (0 fp32, 1 fp64)", dtype);
    return -2;
  }
  if (batch < 0 || n < 1 || m < n) {
    set_error("batched_tall_svd: bad shape batch %d, %d x %d (needs batch >= 0, m >= n >= 1)",
              batch, m, n);
    return -2;
  }
  if (n > kBatchedMaxN) {
    set_error("batched_tall_svd: n = %d columns, at most %d", n, kBatchedMaxN);
    return -2;
  }
  if ((long)m * n >= (1L << 31)) {
    set_error("batched_tall_svd: %d x %d has 2^31 elements or more", m, n);
    return -2;
  }
  if (panel_rows < 0 || panel_rows % 8 != 0) {
    set_error("batched_tall_svd: panel_rows %d (0: chosen here, else a positive multiple of 8)",
              panel_rows);
    return -2;
  }
  const int P = panel_rows ? panel_rows : svdj_batched_tall_panel_rows(dtype, n, V != nullptr);
  const size_t lds = svdj_batched_tall_lds_bytes(dtype, n, V != nullptr, P);
  if (lds == 0) {
    set_error("batched_tall_svd: panels of %d rows x %d (%s) do not fit in %zu bytes of LDS", P,
              n, dtype == 1 ? "fp64" : "fp32", kBatchedLdsCap);
    return -2;
  }
  if (max_sweeps < 0) {
    set_error("batched_tall_svd: max_sweeps %d < 0", max_sweeps);
    return -2;
  }
  if (batch == 0) return 0;
  if (A == nullptr || S == nullptr || sweeps == nullptr || off == nullptr) {
    set_error("batched_tall_svd: A, S, sweeps and off must not be NULL");
    return -2;
  }
  if (U != nullptr && tau_ws == nullptr) {
    set_error("batched_tall_svd: U wanted but tau_ws is NULL (batch x panels x n elements)");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    return batched_tall_launch<float>(batch, m, n, P, A, sb, sr, sc, U, S, V, tau_ws, tol,
                                      tol_mode, max_sweeps, sweeps, off, lds, st);
  return batched_tall_launch<double>(batch, m, n, P, A, sb, sr, sc, U, S, V, tau_ws, tol,
                                     tol_mode, max_sweeps, sweeps, off, lds, st);
}
