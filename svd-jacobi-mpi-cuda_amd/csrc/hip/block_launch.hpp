// Host side of the block Jacobi step (block.hip), part 2: the launchers.  A
// chain's steps run gram(s) -> evd(s) -> apply(s) on its stream (block_steps_t).
// Every launch_* routine takes the chain and a step index and reads the rest --
// buffers, the step's mode (SVDJ_STEP_*, svdj_hip.h), tolerance, inner sweeps,
// metric, matrix-core mode -- from the Chain record (block_layout.hpp), which
// chain_init fills for a solve and the C entry points of block.hip that run one
// stage alone fill for their launcher.  Only launch_quad_apply takes explicit
// parameters: its hook passes values a solve never uses.
#pragma once
#include "block_apply.hpp"
#include "block_evd.hpp"
#include "block_gram.hpp"
#include "block_layout.hpp"
#include "block_quad.hpp"
#include "common.hpp"
#include "svdj_debug.h"

#include <cmath>
#include <type_traits>

namespace svdj {

// flags: svdj_block_steps' mma word (matrix-core mode | SVDJ_STEPS_*).
template <typename T, int W>
static int chain_init(Chain<T>& c, int m_pad, T* A, int lda, T* V, int n_v, int ldv, T* D,
                      const int32_t* pairs, int P, int steps, const int32_t* modes, double tol,
                      int tol_mode, int max_inner, void* ws, size_t ws_bytes, uint32_t* metric,
                      int flags, hipStream_t st, int group_blocks = 0) {
  const int mma = flags & SVDJ_MMA_MASK;
  const bool quad = has_quad_steps(modes, steps);
  if (group_blocks < 0) {
    set_error("group_blocks %d must be >= 0", group_blocks);
    return -2;
  }
  if (group_blocks && quad) {  // the quad kernels keep one metric
    set_error("quad steps are not part of the grouped path (group_blocks %d)", group_blocks);
    return -2;
  }
  if (quad && !has_quad(sizeof(T), W)) {
    set_error("quad steps need fp32 data and W = 64");
    return -3;
  }
  const size_t need = solve_ws_bytes<T>(W, P, m_pad, quad);
  if (ws_bytes < need) {
    set_error("workspace too small: %zu < %zu", ws_bytes, need);
    return -4;
  }
  if (mma != SVDJ_MMA_NATIVE && sizeof(T) != 4) {
    set_error("split-bf16 matrix-core modes need fp32 data");
    return -3;
  }
  if (sizeof(T) == 4 && W == 64 && lda % 4) {  // gram_cross_f32_kernel's 16-byte loads
    set_error("fp32 W = 64 needs lda %% 4 == 0, got %d", lda);
    return -2;
  }
  c = Chain<T>{};
  c.m_pad = m_pad; c.lda = lda; c.n_v = n_v; c.ldv = ldv; c.P = P; c.steps = steps;
  c.A = A; c.V = V; c.D = D; c.pairs = pairs; c.modes = modes; c.st = st;
  c.tol = tol; c.tol_mode = tol_mode; c.max_inner = max_inner; c.metric = metric; c.mma = mma;
  c.group_blocks = group_blocks;
  c.gram_np = (flags & SVDJ_STEPS_GRAM2) ? 2 : 3;
  c.shared = (flags & SVDJ_STEPS_SHARED_GPU) != 0;
  c.g = make_geometry(W, P, m_pad, V ? n_v : 0, mma);
  solve_layout(c, ws, W, quad);
  return 0;
}

// Quad step s (steps s, s+1 fused; see "quad step"): gram (launch_quad_gram),
// then evd 1, T1, update, evd 2, T (launch_quad_chain) on the chain's stream.
template <typename T>
static bool quad_step_ok(const Chain<T>& c, int s) {
  if (c.P % 2 || s + 1 >= c.steps || step_mode(c.modes, s + 1) != SVDJ_STEP_QUAD_SECOND) {
    set_error("quad step %d: needs an even pair count (%d) and a following mode-5 step", s, c.P);
    return false;
  }
  return true;
}

// f(np) with the number of bf16 parts, 2 or (any other value) 3, as a
// compile-time constant: decltype(np)::value.
template <typename F>
static void with_parts(int np, F&& f) {
  if (np == 2) return f(std::integral_constant<int, 2>{});
  f(std::integral_constant<int, 3>{});
}

// The six cross Grams of quad step s into c.qslabs (c.g.qgch row chunks).
template <typename T, int W>
static int launch_quad_gram(const Chain<T>& c, int s) {
  if constexpr (sizeof(T) == 4 && W == 64) {
    const int32_t* pr = c.pairs + (size_t)s * c.P * 2;
    with_parts(c.gram_np, [&](auto np) {
      hipLaunchKernelGGL((gram_quad_kernel<0, decltype(np)::value>), dim3(c.P / 2, c.g.qgch),
                         dim3(kGramQThreads), 0, c.st, c.A, c.lda, c.m_pad, pr, c.P, c.g.qgrows,
                         c.qslabs);
    });
    SVDJ_LAUNCH_CHECK();
    return 0;
  } else {
    (void)c; (void)s;
    set_error("quad steps need fp32 data and W = 64");
    return -3;
  }
}

// Everything of quad step s after its Gram, from the slabs in c.qslabs: evd 1,
// T1, update, evd 2, T.  (Also what svdj_quad_chain runs, on slabs given by
// its caller.)
template <typename T, int W>
static int launch_quad_chain(const Chain<T>& c, int s) {
  if constexpr (sizeof(T) == 4 && W == 64) {
    const int b = s & 1;
    const int32_t* pr = c.pairs + (size_t)s * c.P * 2;
    const int32_t* pr1 = pr + 2 * c.P;
    // many row chunks (few quads): sum them once, wide, for both consumers
    const bool red = c.g.qgch > 4;
    const float* gs = red ? c.qred : c.qslabs;
    const int gn = red ? 1 : c.g.qgch;
    if (red) {
      hipLaunchKernelGGL(slab_reduce_kernel, dim3(3 * c.P, 64 * 64 / 4 / kRedThreads),
                         dim3(kRedThreads), 0, c.st, c.qslabs, c.g.qgch, c.qred);
      SVDJ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((evd_cross_kernel<float, 64>), dim3(c.P), dim3(cross_threads<64>()), 0, c.st,
                       pr, gs, gn, c.D, c.rec, c.nsteps, c.skip1[b], (float)c.tol,
                       c.tol_mode, c.max_inner, c.metric);
    SVDJ_LAUNCH_CHECK();
    constexpr int R = 8;
    // 1024 threads: one workgroup per pair (phase 1) / two (phase 2), so each
    // pair's rotation records are staged 1-2 times instead of 4-8 (128-pair
    // quad step 832 -> 824 us, profiles/r5_ab)
    constexpr int QBT = 1024, QBW = QBT / SVDJ_WAVE;
    // below 64 pairs the Q builds are on the latency path: 2 rows per lane
    // (16384^2 rank plans, ms per sweep: P = 4 76.9 -> 72.5, P = 2 131.9 ->
    // 130.0, profiles/r5_quad2/reduce)
    const bool lat = c.P < 64;
    static const int qb1 = svdj_debug_knob("qb1_threads", 512);  // A/B only (svdj_debug.h)
    if (lat)
      hipLaunchKernelGGL((qbuild_quad_kernel<1, 2, QBT>), dim3(c.P, 128 / (2 * QBW)), dim3(QBT), 0,
                         c.st, c.rec, c.nsteps, c.skip1[b], c.T1);
    else if (qb1 == 512)  // two workgroups per pair: all CUs busy at 128 pairs
      hipLaunchKernelGGL((qbuild_quad_kernel<1, R, 512>), dim3(c.P, 128 / (R * 8)), dim3(512), 0,
                         c.st, c.rec, c.nsteps, c.skip1[b], c.T1);
    else
      hipLaunchKernelGGL((qbuild_quad_kernel<1, R, QBT>), dim3(c.P, 128 / (R * QBW)), dim3(QBT), 0,
                         c.st, c.rec, c.nsteps, c.skip1[b], c.T1);
    SVDJ_LAUNCH_CHECK();
    // 512 threads: 16384^2 -27 ms, 4096^2 -1 ms against 256 (profiles/r6_chain)
    static const int updt = svdj_debug_knob("upd_threads", 512);  // A/B only (svdj_debug.h)
    if (updt == 512)
      hipLaunchKernelGGL(quad_update_kernel<512>, dim3(c.P, 2), dim3(512), 0, c.st,
                         gs + (size_t)c.P * gn * 64 * 64, gn, c.T1, c.upd);
    else
      hipLaunchKernelGGL(quad_update_kernel<256>, dim3(c.P, 2), dim3(256), 0, c.st,
                         gs + (size_t)c.P * gn * 64 * 64, gn, c.T1, c.upd);
    SVDJ_LAUNCH_CHECK();
    hipLaunchKernelGGL((evd_cross_kernel<float, 64>), dim3(c.P), dim3(cross_threads<64>()), 0, c.st,
                       pr1, c.upd, 1, c.D, c.rec, c.nsteps, c.skip2[b], (float)c.tol, c.tol_mode,
                       c.max_inner, c.metric);
    SVDJ_LAUNCH_CHECK();
    // the split T is written directly (no tsplit pass)
    with_parts(svdj_mma_parts(c.mma), [&](auto np) {
      constexpr int NP = decltype(np)::value;
      if (lat)
        hipLaunchKernelGGL((qbuild_quad_kernel<2, 2, QBT, NP>), dim3(c.P, 256 / (2 * QBW)),
                           dim3(QBT), 0, c.st, c.rec, c.nsteps, c.skip2[b], c.T1, c.Ts[b]);
      else
        hipLaunchKernelGGL((qbuild_quad_kernel<2, R, QBT, NP>), dim3(c.P, 256 / (R * QBW)),
                           dim3(QBT), 0, c.st, c.rec, c.nsteps, c.skip2[b], c.T1, c.Ts[b]);
    });
    SVDJ_LAUNCH_CHECK();
    return 0;
  } else {
    (void)c; (void)s;
    set_error("quad steps need fp32 data and W = 64");
    return -3;
  }
}

template <typename T, int W>
static int launch_quad_gram_evd(const Chain<T>& c, int s) {
  if (sizeof(T) == 4 && W == 64 && !quad_step_ok(c, s)) return -2;
  const int rc = launch_quad_gram<T, W>(c, s);
  return rc ? rc : launch_quad_chain<T, W>(c, s);
}

// Gram + EVD of step s (Q and the skip flags are double-buffered so evd(s+1)
// never overwrites what apply(s) may still read).
// Dispatch order of the row chunks (SVDJ_DEBUG stream_order, bit 0: cross
// Gram chunks last-first, bit 1: the apply's V chunks before A's).
// Default 2: V first, so A -- which the next step's Gram reads -- holds the
// most recently written lines (single-stream 16384^2 step 642 -> 614 us,
// bitwise the same result; neutral with two concurrent chains).
static int stream_order() {
  static const int v = svdj_debug_knob("stream_order", 2);
  return v;
}

// The Gram of step s (cross or full) into c.slabs (c.g.gchunks row chunks).
template <typename T, int W>
static int launch_gram(const Chain<T>& c, int s) {
  const int32_t* pr = c.pairs + (size_t)s * c.P * 2;
  const int full = step_mode(c.modes, s) == SVDJ_STEP_FULL;
  constexpr int XS = gram_xsplit<T, W>();
  if (full) {
    if constexpr (XS > 1)  // see GRAM_SPLIT
      hipLaunchKernelGGL((gram_kernel<T, W, GRAM_SPLIT>), dim3(c.P, c.g.gchunks, 3 * XS),
                         dim3(kGramThreads), 0, c.st, c.A, c.lda, c.m_pad, pr, c.g.grows, c.slabs);
    else
      hipLaunchKernelGGL((gram_kernel<T, W, GRAM_FULL>), dim3(c.P, c.g.gchunks),
                         dim3(kGramThreads), 0, c.st, c.A, c.lda, c.m_pad, pr, c.g.grows, c.slabs);
  } else if constexpr (sizeof(T) == 4 && W == 64) {  // coalesced loads, LDS transpose
    hipLaunchKernelGGL((gram_cross_f32_kernel<GRAM_CROSS>), dim3(c.P, c.g.gchunks),
                       dim3(kGramThreads), 0, c.st, c.A, c.lda, c.m_pad, pr, c.g.grows, c.slabs,
                       stream_order() & 1);
  } else {
    hipLaunchKernelGGL((gram_kernel<T, W, GRAM_CROSS>), dim3(c.P, c.g.gchunks, XS),
                       dim3(kGramThreads), 0, c.st, c.A, c.lda, c.m_pad, pr, c.g.grows, c.slabs);
  }
  SVDJ_LAUNCH_CHECK();
  return 0;
}

// Everything of step s (cross or full) after its Gram, from the slabs in
// c.slabs: the EVD and, for SVDJ_STEP_CROSS_ONLY, the chunk pre-sum and the Q
// build.  (Also what svdj_evd_alone runs, on slabs given by its caller.)
template <typename T, int W>
static int launch_evd(const Chain<T>& c, int s) {
  const int b = s & 1;
  const int32_t* pr = c.pairs + (size_t)s * c.P * 2;
  const int mode = step_mode(c.modes, s);
  const int full = mode == SVDJ_STEP_FULL;
  if (mode == SVDJ_STEP_CROSS_ONLY) {
    // many row chunks (few pairs per step: the 8-GPU plans read 32): sum them
    // once, wide, instead of on the EVD's critical path (one workgroup per
    // pair reading every chunk); bitwise the same sums (slab_reduce_kernel)
    const T* gs = c.slabs;
    int gn = c.g.gchunks;
    if constexpr (sizeof(T) == 4 && W == 64) {
      static const int red_from = svdj_debug_knob("cross_reduce_chunks", 9);  // A/B only
      if (gn >= red_from) {
        hipLaunchKernelGGL(slab_reduce_kernel, dim3(c.P, W * W / 4 / kRedThreads), dim3(kRedThreads),
                           0, c.st, c.slabs, gn, c.xsum);
        SVDJ_LAUNCH_CHECK();
        gs = c.xsum;
        gn = 1;
      }
    }
    hipLaunchKernelGGL((evd_cross_kernel<T, W>), dim3(c.P), dim3(cross_threads<W>()), 0, c.st, pr,
                       gs, gn, c.D, c.rec, c.nsteps, c.skipb[b], (T)c.tol, c.tol_mode, c.max_inner,
                       c.metric, c.group_blocks);
    SVDJ_LAUNCH_CHECK();
    constexpr int RL = W == 64 ? 16 : 8;  // one workgroup per pair
    // 16 rows per lane from 64 pairs per step; at 32 pairs 4 rows per lane is
    // faster (1 GPU 8192^2 709 -> 672 ms, 16384^2 P=2 plan 171.4 -> 169.1 ms per
    // sweep; 1 GPU 16384^2 (64 pairs) equal at 4/8/16, profiles/r3_s3/qbuild)
    // below 16 pairs (8-GPU plans) 2 rows per lane: a shorter rotation chain
    // per lane on the latency path (16384^2 P = 8: 44.1-44.5 -> 43.6-43.7 ms
    // per sweep, profiles/r5_ab/qb2)
    if (c.P >= 64)
      hipLaunchKernelGGL((qbuild_kernel<T, W, RL>), dim3(c.P, qbuild_blocks<W, RL>()),
                         dim3(kQbThreads), 0, c.st, c.rec, c.nsteps, c.skipb[b], c.Qb[b]);
    else if (W == 64 && c.P < 16)
      hipLaunchKernelGGL((qbuild_kernel<T, W, 2>), dim3(c.P, qbuild_blocks<W, 2>()),
                         dim3(kQbThreads), 0, c.st, c.rec, c.nsteps, c.skipb[b], c.Qb[b]);
    else
      hipLaunchKernelGGL((qbuild_kernel<T, W, 4>), dim3(c.P, qbuild_blocks<W, 4>()),
                         dim3(kQbThreads), 0, c.st, c.rec, c.nsteps, c.skipb[b], c.Qb[b]);
  } else if (mode == SVDJ_STEP_CROSS_BIP)
    hipLaunchKernelGGL((evd_kernel<T, W, EVD_BIP>), dim3(c.P), dim3(kEvdThreads), 0, c.st, pr,
                       0, c.slabs, c.g.gchunks, c.D, c.Qb[b], c.skipb[b], (T)c.tol, c.tol_mode,
                       c.max_inner, c.metric, c.group_blocks);
  else
    hipLaunchKernelGGL((evd_kernel<T, W, EVD_CYCLIC>), dim3(c.P), dim3(kEvdThreads), 0, c.st,
                       pr, full, c.slabs, c.g.gchunks, c.D, c.Qb[b], c.skipb[b], (T)c.tol,
                       c.tol_mode, c.max_inner, c.metric, c.group_blocks);
  SVDJ_LAUNCH_CHECK();
  return 0;
}

template <typename T, int W>
static int launch_gram_evd(const Chain<T>& c, int s) {
  const int mode = step_mode(c.modes, s);
  if (mode == SVDJ_STEP_QUAD_SECOND) return 0;  // done by the quad's first step
  if (mode == SVDJ_STEP_QUAD) return launch_quad_gram_evd<T, W>(c, s);
  const int rc = launch_gram<T, W>(c, s);
  return rc ? rc : launch_evd<T, W>(c, s);
}

// The apply of quad step s (T-stationary, persistent: apply_quad_ts_kernel<np>
// on `grid` workgroups) on A and V with T - I from c.Ts, for the c.P / 2 quads
// of the step's pairs.  cheap_tol: the bound on |T - I| of a cheap k half
// (np == 2 takes the kernel's default); work: its work counters, or null.
// (Also what svdj_apply_quad runs, on a T given by its caller.)
static int launch_quad_apply(const Chain<float>& c, int s, int np, int grid, float cheap_tol,
                             uint32_t* work) {
  const int b = s & 1;
  const int32_t* pr = c.pairs + (size_t)s * c.P * 2;
  const int nq = c.P / 2, at = c.m_pad / 32, vt = c.V ? c.n_v / 32 : 0;
  if (np == 3)
    hipLaunchKernelGGL((apply_quad_ts_kernel<3>), dim3(grid), dim3(kQuadTsThreads), 0, c.st, c.A,
                       c.lda, at, c.V, c.ldv, vt, pr, nq, c.Ts[b], c.skip1[b], c.skip2[b], work,
                       cheap_tol);
  else
    hipLaunchKernelGGL((apply_quad_ts_kernel<2>), dim3(grid), dim3(kQuadTsThreads), 0, c.st, c.A,
                       c.lda, at, c.V, c.ldv, vt, pr, nq, c.Ts[b], c.skip1[b], c.skip2[b], work);
  SVDJ_LAUNCH_CHECK();
  return 0;
}

template <typename T, int W>
static int launch_apply(const Chain<T>& c, int s) {
  const int b = s & 1;
  const int32_t* pr = c.pairs + (size_t)s * c.P * 2;
  const int nv = c.V ? c.n_v : 0, ych = c.V ? c.g.v_chunks : 0;
  const int mode = step_mode(c.modes, s), parts = svdj_mma_parts(c.mma);
  if (mode == SVDJ_STEP_QUAD_SECOND) return 0;
  if (mode == SVDJ_STEP_QUAD) {
    if constexpr (sizeof(T) == 4 && W == 64) {
      if (!parts) {
        set_error("quad steps run the split-bf16 apply (mma 1 or 2), got %d", c.mma);
        return -3;
      }
      // cheap k halves: |T - I| <= 2^-7 (A/B only: SVDJ_DEBUG cheap_log2, svdj_debug.h)
      static const float cheap_tol = ldexpf(1.0f, -svdj_debug_knob("cheap_log2", 7));
      // persistent grid (A/B override: SVDJ_DEBUG apply_grid)
      static const int grid_knob = svdj_debug_knob("apply_grid", 0);
      const int grid =
          grid_knob > 0 ? grid_knob : c.shared ? quad_ts_grid_shared(c.P / 2) : kQuadTsGrid;
      return launch_quad_apply(c, s, parts, grid, cheap_tol, c.metric ? c.metric + 6 : nullptr);
    } else {
      set_error("quad steps need fp32 data and W = 64");
      return -3;
    }
  }
  const dim3 grid(c.P, c.g.a_chunks + ych);
  if constexpr (sizeof(T) == 4) {
    if (parts) {
      with_parts(parts, [&](auto np) {
        hipLaunchKernelGGL((apply_split_kernel<W, decltype(np)::value>), grid, dim3(kApplyThreads),
                           0, c.st, c.A, c.lda, c.g.a_chunks, c.g.rows_a, c.m_pad, c.V, c.ldv,
                           c.g.rows_v, nv, pr, c.Qb[b], c.skipb[b], (stream_order() >> 1) & 1);
      });
      SVDJ_LAUNCH_CHECK();
      return 0;
    }
  }
  hipLaunchKernelGGL((apply_kernel<T, W>), grid, dim3(apply_threads<T, W>()), 0, c.st, c.A, c.lda,
                     c.g.a_chunks, c.g.rows_a, c.m_pad, c.V, c.ldv, c.g.rows_v, nv, pr, c.Qb[b],
                     c.skipb[b]);
  SVDJ_LAUNCH_CHECK();
  return 0;
}

// Step pipeline on the chain's stream: gram(s) -> evd(s) -> apply(s).
//
// c.mma: SVDJ_MMA_NATIVE = native matrix cores for the data type (f32 / f64 MFMA),
//        SVDJ_MMA_BF16X6 = fp32 data on bf16 MFMA, 3-way split (fp32-level accuracy),
//        SVDJ_MMA_BF16X3 = fp32 data on bf16 MFMA, 2-way split (~2^-17, fast mode).
// Both split modes run in delta form, Y = X + X (Q - I) (apply_split_kernel).
// Measured on MI355X (bench.py accuracy block, profiles/r3_s3/bf16x6,
// profiles/r4_accuracy): BF16X6 matches the f32 MFMA path in U/V orthogonality
// and sigma error (16384^2: 2.43e-7 both), its residual is 1.37-1.55e-5 vs
// 1.03-1.05e-5, and it is 12-23 % faster per sweep for W = 64, so it is the
// fp32 default there (svdj_choose_mma).  Deferring V's rotation to a side
// stream (it is not needed by the next Gram) was measured neutral on one
// stream and 22 % slower with two chains (8192^2, round 4): not kept.
template <typename T, int W>
static int block_steps_t(const Chain<T>& c) {
  for (int s = 0; s < c.steps; ++s) {
    int rc = launch_gram_evd<T, W>(c, s);
    if (!rc) rc = launch_apply<T, W>(c, s);
    if (rc) return rc;
  }
  return 0;
}

// f(T{}, w) for the data type (0 fp32, 1 fp64) and block width, the width as
// a compile-time constant (decltype(w)::value); -3 for any other pair.
template <typename F>
static int dispatch_tw(int dtype, int W, F&& f) {
  if (dtype == 0 && W == 32) return f(float{}, std::integral_constant<int, 32>{});
  if (dtype == 0 && W == 64) return f(float{}, std::integral_constant<int, 64>{});
  if (dtype == 1 && W == 32) return f(double{}, std::integral_constant<int, 32>{});
  if (dtype == 1 && W == 64) return f(double{}, std::integral_constant<int, 64>{});
  set_error("unsupported (dtype=%d, W=%d); supported: W in {32, 64}", dtype, W);
  return -3;
}

}  // namespace svdj
