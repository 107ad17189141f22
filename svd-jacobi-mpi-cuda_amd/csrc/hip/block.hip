// Block one-sided Jacobi step on MFMA (the performance path).
//
// The reference rotates one column pair at a time with a memory-bound Givens
// kernel (reference main.cu:139-147) driven by host dot products
// (main.cu:698-707).  On CDNA4 the same sweep is re-blocked so every byte of
// A and V moved through HBM feeds matrix-core work:
//
//   columns are grouped in blocks of W; a step processes P disjoint block
//   pairs (bi, bj) with X = [A_bi A_bj] (m x 2W):
//     gram  : C = A_bi^T A_bj (cross) or G = X^T X (full), MFMA, split over
//             rows into partial slabs (deterministic, no float atomics);
//     evd   : G = [[D_bi, C], [C^T, D_bj]] -> Q^T G Q = Lambda by cyclic
//             parallel Jacobi held entirely in LDS (one 1024-thread WG per
//             pair); the convergence value max|g_pq|/sqrt(g_pp g_qq) of the
//             reference (main.cu:710) becomes the stop test;
//     apply : X <- X Q and [V_bi V_bj] <- [..] Q in place, MFMA, computed
//             transposed (Out^T = Q^T X^T) so loads AND stores are
//             128-byte coalesced column segments.
//
// Blocks are kept internally orthogonal (every step fully diagonalises its
// pair), so only the W x W cross Gram is needed per step; the diagonal blocks
// are the tracked squared column norms D.  The first step of a sweep uses the
// full Gram, which re-measures every within-block angle from the data.
//
// One translation unit, cut by stage into headers: block_gram.hpp,
// block_evd.hpp (the EVD kernels and the Q build), block_apply.hpp,
// block_quad.hpp (the fused two-step kernels), block_layout.hpp (geometry,
// Chain, workspace layouts) and block_launch.hpp (the launchers).  This file
// holds the C entry points.
#include "block_launch.hpp"
#include "block_layout.hpp"
#include "common.hpp"
#include "svdj_hip.h"
#include "svdj_stop.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace svdj;

// Cross-step EVD ordering for a step of `pairs` pairs of W-wide blocks
// (models/block.py choose_inner_order, measurements there): cross-only
// (low-latency EVD + row-parallel Q build) for fp32 W = 64 and for fp64
// W = 64 with more than 16 pairs, else bipartite.  The inner_order codes
// (SVDJ_INNER_*) of svdj_block_solve / svdj_dist_problem.
extern "C" int svdj_choose_inner_order(int dtype, int W, int pairs) {
  if (W != 64) return SVDJ_INNER_BIPARTITE;
  return (dtype == 0 || pairs > 16) ? SVDJ_INNER_CROSS : SVDJ_INNER_BIPARTITE;
}

// Default matrix-core mode ("auto") for data type `dtype` (0 fp32, 1 fp64)
// and block width W (models/block.py choose_mma): the split-bf16 apply for
// fp32 W = 64; W = 32 steps stay on f32 MFMA (4096^2 P=8
// rank plan, W = 32: 8.55 vs 9.61 ms per sweep with the split).
extern "C" int svdj_choose_mma(int dtype, int W) {
  return (dtype == 0 && W == 64) ? SVDJ_MMA_BF16X6 : SVDJ_MMA_NATIVE;
}

extern "C" size_t svdj_block_workspace_bytes(int dtype, int W, int P, int m_pad, int quad) {
  return dtype == 1 ? solve_ws_bytes<double>(W, P, m_pad, quad != 0)
                    : solve_ws_bytes<float>(W, P, m_pad, quad != 0);
}

static int check_dims(int m_pad, int lda, const void* V, int n_v, int ldv, int mma) {
  if (m_pad <= 0 || m_pad % SVDJ_ROW_ALIGN || lda < m_pad) {
    set_error("bad m_pad/lda %d/%d", m_pad, lda);
    return -2;
  }
  if (V && (n_v <= 0 || n_v % SVDJ_ROW_ALIGN || ldv < n_v)) {
    set_error("bad n_v/ldv %d/%d", n_v, ldv);
    return -2;
  }
  if (mma < 0 || mma > 2) {
    set_error("bad matrix-core mode %d", mma);
    return -2;
  }
  return 0;
}

extern "C" int svdj_block_steps_grouped(int dtype, int W, int m_pad, void* A, int lda, void* V,
                                        int n_v, int ldv, void* D, const int32_t* pairs, int P,
                                        int steps, const int32_t* modes, double tol, int tol_mode,
                                        int max_inner, void* ws, size_t ws_bytes, uint32_t* metric,
                                        int group_blocks, int mma, void* stream) {
  // mma: the apply's matrix-core mode | SVDJ_STEPS_* (svdj_hip.h; chain_init)
  int rc = check_dims(m_pad, lda, V, n_v, ldv, mma & SVDJ_MMA_MASK);
  if (rc) return rc;
  if (tol_mode != 0 && tol_mode != 1) {
    set_error("bad tol_mode %d (0 relative, 1 absolute)", tol_mode);
    return -2;
  }
  if (P <= 0 || steps < 0) return 0;
  return dispatch_tw(dtype, W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W_ = decltype(w)::value;
    Chain<T> c;
    const int err = chain_init<T, W_>(c, m_pad, (T*)A, lda, (T*)V, n_v, ldv, (T*)D, pairs, P,
                                      steps, modes, tol, tol_mode, max_inner, ws, ws_bytes, metric,
                                      mma, (hipStream_t)stream, group_blocks);
    return err ? err : block_steps_t<T, W_>(c);
  });
}

extern "C" int svdj_block_steps(int dtype, int W, int m_pad, void* A, int lda, void* V, int n_v,
                                int ldv, void* D, const int32_t* pairs, int P, int steps,
                                const int32_t* modes, double tol, int tol_mode, int max_inner,
                                void* ws, size_t ws_bytes, uint32_t* metric, int mma,
                                void* stream) {
  return svdj_block_steps_grouped(dtype, W, m_pad, A, lda, V, n_v, ldv, D, pairs, P, steps, modes,
                                  tol, tol_mode, max_inner, ws, ws_bytes, metric, 0, mma, stream);
}

extern "C" int svdj_block_solve(int dtype, int W, int m_pad, void* A, int lda, void* V, int n_v,
                                int ldv, void* D, int ncols, double tol, int tol_mode,
                                int max_inner, int max_sweeps, int inner_order, void* ws,
                                size_t ws_bytes, uint32_t* metric, double* hist, int mma,
                                int stop_rule, void* stream) {
  if (W <= 0 || ncols % W) {
    set_error("ncols %d not a multiple of W %d", ncols, W);
    return -2;
  }
  const int nb = ncols / W;
  if (nb < 2 || (nb & 1)) {
    set_error("block count %d must be even and >= 2", nb);
    return -2;
  }
  const int P = nb / 2, steps = nb - 1;
  std::vector<int32_t> h((size_t)steps * P * 2);
  for (int r = 0; r < steps; ++r) {
    int32_t* o = h.data() + (size_t)r * P * 2;
    o[0] = r;
    o[1] = nb - 1;
    for (int k = 1; k < P; ++k) {
      int a = (r + k) % (nb - 1), b = (r - k + nb - 1) % (nb - 1);
      o[2 * k] = a < b ? a : b;
      o[2 * k + 1] = a < b ? b : a;
    }
  }
  if (inner_order == SVDJ_INNER_AUTO) inner_order = svdj_choose_inner_order(dtype, W, P);
  if (inner_order < SVDJ_INNER_CYCLIC || inner_order > SVDJ_INNER_CROSS) {
    set_error("inner_order %d (0 cyclic, 1 bipartite, 2 cross, 3 auto)", inner_order);
    return -2;
  }
  std::vector<int32_t> modes(steps, svdj_cross_step_mode(inner_order));
  modes[0] = SVDJ_STEP_FULL;
  hipStream_t st = (hipStream_t)stream;
  int32_t* dpairs = nullptr;
  SVDJ_HIP_CHECK(hipMallocAsync((void**)&dpairs, h.size() * sizeof(int32_t), st));
  SVDJ_HIP_CHECK(hipMemcpyAsync(dpairs, h.data(), h.size() * sizeof(int32_t),
                                hipMemcpyHostToDevice, st));
  int sweeps = 0, rc = 0;
  uint32_t hm[6];
  // underflow floor of this solve (metric[2..3])
  rc = svdj_set_norm_floor_scaled(dtype, m_pad, D, ncols, metric, stream);
  for (int sw = 0; sw < max_sweeps && rc >= 0; ++sw) {
    if (svdj_reset_metric(metric, stream) != 0) { rc = -100; break; }
    rc = svdj_block_steps(dtype, W, m_pad, A, lda, V, n_v, ldv, D, dpairs, P, steps,
                          modes.data(), tol, tol_mode, max_inner, ws, ws_bytes, metric, mma,
                          stream);
    if (rc) break;
    if (hipMemcpyAsync(hm, metric, sizeof(hm), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      set_error("metric readback failed");
      rc = -100;
      break;
    }
    float mx, ms;
    memcpy(&mx, &hm[0], sizeof(float));
    memcpy(&ms, &hm[4], sizeof(float));
    if (hist) hist[sw] = mx;
    sweeps = sw + 1;
    if (svdj_sweep_converged_inline(mx, ms, hm[1], hm[5], tol, tol_mode, stop_rule)) break;
  }
  (void)hipFreeAsync(dpairs, st);
  return rc ? rc : sweeps;
}

// The Gram of a single step alone (tests / kernel A/B): launch_gram on the
// device pair list with the given row chunking, every case of it -- fp32 and
// fp64, W = 32 and 64, mode SVDJ_STEP_FULL (slabs P x nchunk x 2W x 2W of
// [A_bi A_bj]^T [A_bi A_bj]) or SVDJ_STEP_CROSS (P x nchunk x W x W of
// A_bi^T A_bj; the other cross modes run the same Gram).
extern "C" int svdj_gram(int dtype, int W, int mode, const void* A, int lda, int m_pad,
                         const int32_t* pairs, int P, int rows_per_chunk, void* slabs,
                         void* stream) {
  if (m_pad <= 0 || m_pad % SVDJ_ROW_ALIGN || lda < m_pad || P <= 0 || rows_per_chunk <= 0 ||
      rows_per_chunk % SVDJ_ROW_ALIGN || !A || !pairs || !slabs) {
    set_error("svdj_gram: bad m_pad/lda/P/rows %d/%d/%d/%d or a null pointer", m_pad, lda, P,
              rows_per_chunk);
    return -2;
  }
  if (mode != SVDJ_STEP_CROSS && mode != SVDJ_STEP_FULL) {
    set_error("svdj_gram: mode %d (SVDJ_STEP_CROSS or SVDJ_STEP_FULL)", mode);
    return -2;
  }
  if (dtype == 0 && W == 64 && lda % 4) {  // 16-byte loads along the rows of a column
    set_error("svdj_gram: lda %d must be a multiple of 4", lda);
    return -2;
  }
  return dispatch_tw(dtype, W, [&](auto t, auto w) {
    using T = decltype(t);
    const int32_t modes[1] = {mode};  // c.modes: read by launch_gram below, not after it
    Chain<T> c{};  // the fields launch_gram reads
    c.A = const_cast<T*>((const T*)A);  // only read by the Gram
    c.lda = lda; c.m_pad = m_pad; c.pairs = pairs; c.P = P; c.steps = 1; c.modes = modes;
    c.st = (hipStream_t)stream;
    c.g.grows = rows_per_chunk;
    c.g.gchunks = (m_pad + rows_per_chunk - 1) / rows_per_chunk;
    c.slabs = (T*)slabs;
    return launch_gram<T, decltype(w)::value>(c, 0);
  });
}

// The cross Gram alone: svdj_gram with SVDJ_STEP_CROSS.
extern "C" int svdj_gram_cross(int dtype, int W, const void* A, int lda, int m_pad,
                               const int32_t* pairs, int P, int rows_per_chunk, void* slabs,
                               void* stream) {
  return svdj_gram(dtype, W, SVDJ_STEP_CROSS, A, lda, m_pad, pairs, P, rows_per_chunk, slabs,
                   stream);
}

// The six cross Grams of a quad step (fp32, W = 64) alone (tests / kernel
// A/B): pairs = the step's P pairs in quad order ((a,c),(b,d) per quad);
// slabs (3P x nchunk x W x W): [0, P) the pairs' Grams, then C_ad, C_bc, C_ab,
// C_cd of every quad (gram_quad_kernel through launch_quad_gram).
extern "C" int svdj_gram_quad(const void* A, int lda, int m_pad, const int32_t* pairs, int P,
                              int rows_per_chunk, void* slabs, int parts, void* stream) {
  if (m_pad <= 0 || m_pad % SVDJ_ROW_ALIGN || lda < m_pad || lda % 4 || P <= 0 || P % 2 ||
      rows_per_chunk <= 0 || rows_per_chunk % SVDJ_ROW_ALIGN || (parts != 2 && parts != 3)) {
    set_error("svdj_gram_quad: bad m_pad/lda/P/rows/parts %d/%d/%d/%d/%d", m_pad, lda, P,
              rows_per_chunk, parts);
    return -2;
  }
  Chain<float> c{};  // the fields launch_quad_gram reads
  c.A = const_cast<float*>((const float*)A);  // only read by the Gram
  c.lda = lda; c.m_pad = m_pad; c.pairs = pairs; c.P = P; c.st = (hipStream_t)stream;
  c.g.qgrows = rows_per_chunk;
  c.g.qgch = (m_pad + rows_per_chunk - 1) / rows_per_chunk;
  c.gram_np = parts;
  c.qslabs = (float*)slabs;
  return launch_quad_gram<float, 64>(c, 0);
}

// The quad step's apply alone (tests / kernel A/B): [a b c d] <- [a b c d] T
// on A (m_pad rows) and V (n_v rows, or NULL) for the nq quads of `pairs`
// (2 nq pairs in quad order (a,c),(b,d)), T - I given split into np bf16
// parts in the ts_frag layout; skip1 / skip2 (2 nq flags each): a quad is
// skipped when all four of its flags are set.  apply_quad_ts_kernel<np> on
// `grid` workgroups through launch_quad_apply; cheap_tol = 2^-cheap_log2;
// work (device uint32[2], or NULL): the kernel's work counters, accumulated.
extern "C" int svdj_apply_quad(void* A, int lda, int m_pad, void* V, int n_v, int ldv,
                               const int32_t* pairs, int nq, const void* Ts,
                               const int32_t* skip1, const int32_t* skip2, int np, int grid,
                               int cheap_log2, uint32_t* work, void* stream) {
  int rc = check_dims(m_pad, lda, V, n_v, ldv, 0);
  if (rc) return rc;
  if (lda % 4 || (V && ldv % 4)) {  // the tile DMA moves 16 bytes per lane
    set_error("svdj_apply_quad: lda/ldv %d/%d must be multiples of 4", lda, ldv);
    return -2;
  }
  if ((np != 2 && np != 3) || grid < 1 || nq < 1 || cheap_log2 < 0 || cheap_log2 > 126 || !A ||
      !pairs || !Ts || !skip1 || !skip2) {
    set_error("svdj_apply_quad: bad np/grid/nq/cheap_log2 %d/%d/%d/%d or a null pointer", np, grid,
              nq, cheap_log2);
    return -2;
  }
  Chain<float> c{};  // the fields launch_quad_apply reads
  c.A = (float*)A; c.lda = lda; c.m_pad = m_pad; c.V = (float*)V; c.n_v = n_v; c.ldv = ldv;
  c.pairs = pairs; c.P = 2 * nq; c.st = (hipStream_t)stream;
  c.Ts[0] = const_cast<bf16x8*>((const bf16x8*)Ts);  // T and the flags are only read
  c.skip1[0] = const_cast<int32_t*>(skip1);
  c.skip2[0] = const_cast<int32_t*>(skip2);
  return launch_quad_apply(c, 0, np, grid, ldexpf(1.0f, -cheap_log2), work);
}

// The middle of a single step alone (tests): launch_evd -- what a step of
// svdj_block_steps runs after its Gram -- on slabs given by the caller.
//   slabs   device, data type: P x nchunk x W x W (SVDJ_STEP_FULL: 2W x 2W),
//           the layout the Gram kernels write; copied into the workspace's slab area
//   D       squared column norms by block (updated in place), pairs device
//           int32 [P][2], mode SVDJ_STEP_CROSS to SVDJ_STEP_CROSS_ONLY
//   Q       out, P x 2W x 2W (data type; a skipped pair's may stay unwritten)
//   skip    out, int32 [P]
//   ws      svdj_evd_alone_workspace_bytes: the slab area of a step with
//           nchunk row chunks, the rotation records and the step counts
extern "C" size_t svdj_evd_alone_workspace_bytes(int dtype, int W, int P, int nchunk) {
  if ((dtype != 0 && dtype != 1) || (W != 32 && W != 64) || P < 1 || nchunk < 1) return 0;
  return dtype == 1 ? evd_alone_ws_bytes<double>(W, P, nchunk)
                    : evd_alone_ws_bytes<float>(W, P, nchunk);
}

extern "C" int svdj_evd_alone(int dtype, int W, int mode, const void* slabs, int nchunk, void* D,
                              const int32_t* pairs, int P, double tol, int tol_mode, int max_inner,
                              void* Q, int32_t* skip, void* ws, size_t ws_bytes, uint32_t* metric,
                              void* stream) {
  return dispatch_tw(dtype, W, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr int W_ = decltype(w)::value;
    if (mode < 0 || mode > SVDJ_STEP_CROSS_ONLY || P < 1 || nchunk < 1 || max_inner < 0 ||
        (tol_mode != 0 && tol_mode != 1) || !slabs || !D || !pairs || !Q || !skip || !ws ||
        !metric) {
      set_error("svdj_evd_alone: bad mode/P/nchunk/max_inner/tol_mode %d/%d/%d/%d/%d or a null "
                "pointer", mode, P, nchunk, max_inner, tol_mode);
      return -2;
    }
    const int32_t modes[1] = {mode};  // c.modes: must outlive the launch_evd call below
    Chain<T> c{};  // the fields launch_evd reads
    c.P = P; c.steps = 1; c.D = (T*)D; c.pairs = pairs; c.modes = modes;
    c.st = (hipStream_t)stream;
    c.tol = tol; c.tol_mode = tol_mode; c.max_inner = max_inner; c.metric = metric;
    c.g.gchunks = nchunk;
    c.Qb[0] = (T*)Q;
    c.skipb[0] = skip;
    const size_t need = evd_alone_layout(c, ws, W_);
    if (ws_bytes < need) {
      set_error("svdj_evd_alone: workspace too small: %zu < %zu", ws_bytes, need);
      return -2;
    }
    const int full = mode == SVDJ_STEP_FULL;
    const size_t in_bytes = (size_t)P * nchunk * (full ? 4 : 1) * W_ * W_ * sizeof(T);
    SVDJ_HIP_CHECK(hipMemcpyAsync(c.slabs, slabs, in_bytes, hipMemcpyDeviceToDevice, c.st));
    return launch_evd<T, W_>(c, 0);
  });
}

// The middle of a quad step alone (tests; fp32, W = 64): launch_quad_chain --
// what a quad step of svdj_block_steps runs after its Gram -- on slabs given
// by the caller, read in place.
//   slabs   device fp32, 3P x nchunk x 64 x 64 in svdj_gram_quad's order
//   pairs   device int32 [2][P][2]: the SVDJ_STEP_QUAD step's pairs in quad order
//           ((a,c), (b,d) per quad), then those of its second step ((a,d), (b,c))
//   np      parts of the split T: svdj_mma_parts of svdj_block_steps' mma
//   T1      out, fp64 P x 128 x 128; upd out, fp32 P x 64 x 64; Ts out, bf16
//           (P / 2) x 256 x 256 x np (svdj_apply_quad's layout); skip1, skip2
//           out, int32 [P] each
//   ws      svdj_quad_chain_workspace_bytes: the chunk sums, the rotation
//           records and the step counts
extern "C" size_t svdj_quad_chain_workspace_bytes(int P) {
  Chain<float> c{};
  c.P = P;
  return P < 2 || P % 2 ? 0 : quad_chain_layout(c, nullptr);
}

extern "C" int svdj_quad_chain(const void* slabs, int nchunk, void* D, const int32_t* pairs, int P,
                               double tol, int tol_mode, int max_inner, int np, void* T1, void* upd,
                               void* Ts, int32_t* skip1, int32_t* skip2, void* ws, size_t ws_bytes,
                               uint32_t* metric, void* stream) {
  if (P < 2 || P % 2 || nchunk < 1 || max_inner < 0 || (tol_mode != 0 && tol_mode != 1) ||
      (np != 2 && np != 3) || !slabs || !D || !pairs || !T1 || !upd || !Ts || !skip1 || !skip2 ||
      !ws || !metric) {
    set_error("svdj_quad_chain: bad P/nchunk/max_inner/tol_mode/np %d/%d/%d/%d/%d or a null pointer",
              P, nchunk, max_inner, tol_mode, np);
    return -2;
  }
  static const int32_t modes[2] = {SVDJ_STEP_QUAD, SVDJ_STEP_QUAD_SECOND};
  Chain<float> c{};  // the fields launch_quad_chain reads
  c.P = P; c.steps = 2; c.D = (float*)D; c.pairs = pairs; c.modes = modes;
  c.st = (hipStream_t)stream; c.mma = np == 2 ? SVDJ_MMA_BF16X3 : SVDJ_MMA_BF16X6;
  c.tol = tol; c.tol_mode = tol_mode; c.max_inner = max_inner; c.metric = metric;
  const size_t need = quad_chain_layout(c, ws);
  if (ws_bytes < need) {
    set_error("svdj_quad_chain: workspace too small: %zu < %zu", ws_bytes, need);
    return -2;
  }
  c.g.qgch = nchunk;
  c.qslabs = const_cast<float*>((const float*)slabs);  // only read after the Gram
  c.T1 = (double*)T1;
  c.upd = (float*)upd;
  c.Ts[0] = (bf16x8*)Ts;
  c.skip1[0] = skip1;
  c.skip2[0] = skip2;
  if (!quad_step_ok(c, 0)) return -2;
  return launch_quad_chain<float, 64>(c, 0);
}

// Test/diagnostic hook: X <- X Q for ONE column-block pair (blocks 0 and 1 of
// X, 2W columns with leading dimension ld, rows padded to SVDJ_ROW_ALIGN),
// Q row-major 2W x 2W on the device, with the given matrix-core mode: a
// one-pair step of 512-row chunks through launch_apply.
extern "C" int svdj_apply_q(int dtype, int W, int mma, void* X, int rows, int ld, const void* Q,
                            void* stream) {
  if (rows <= 0 || rows % SVDJ_ROW_ALIGN || ld < rows) {
    set_error("bad rows/ld %d/%d", rows, ld);
    return -2;
  }
  static const int32_t hpair[2] = {0, 1};
  static const int32_t hskip[1] = {0};
  hipStream_t st = (hipStream_t)stream;
  int32_t* dbuf = nullptr;
  SVDJ_HIP_CHECK(hipMallocAsync((void**)&dbuf, 3 * sizeof(int32_t), st));
  SVDJ_HIP_CHECK(hipMemcpyAsync(dbuf, hpair, 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SVDJ_HIP_CHECK(hipMemcpyAsync(dbuf + 2, hskip, sizeof(int32_t), hipMemcpyHostToDevice, st));
  int rc = -3;
  if (mma < 0 || mma > 2 || (dtype == 1 && mma != SVDJ_MMA_NATIVE))
    set_error("svdj_apply_q: unsupported dtype=%d W=%d mma=%d", dtype, W, mma);
  else
    rc = dispatch_tw(dtype, W, [&](auto t, auto w) {
      using T = decltype(t);
      // the fields launch_apply reads (no modes: a cross step; no V: A's row
      // chunks only; no metric: only a quad step's apply counts its work)
      Chain<T> c{};
      c.A = (T*)X; c.lda = ld; c.m_pad = rows; c.pairs = dbuf; c.P = 1; c.st = st;
      c.mma = mma;
      c.g.rows_a = 512;
      c.g.a_chunks = (rows + c.g.rows_a - 1) / c.g.rows_a;
      c.Qb[0] = const_cast<T*>((const T*)Q);  // only read by the apply
      c.skipb[0] = dbuf + 2;
      return launch_apply<T, decltype(w)::value>(c, 0);
    });
  (void)hipFreeAsync(dbuf, st);
  return rc;
}
