// Host side of the block Jacobi step (block.hip), part 1: launch geometry,
// the Chain record of one chain of steps, and the workspace layouts.  Host
// code only; includes no kernel header (tools/micro/ws_layout_check.hip checks
// the layouts with no kernel in the program).
#pragma once
#include "common.hpp"
#include "svdj_debug.h"
#include "svdj_hip.h"

namespace svdj {

// ------------------------------------------------------------- host side
struct Geometry {
  int gchunks, grows;  // gram
  int a_chunks, rows_a, v_chunks, rows_v;
  // quad steps (fp32 W = 64): gram row chunks, apply row chunks
  int qgch, qgrows;
};

// Quad-step geometry: row chunks of gram_quad_kernel (its slabs are summed
// by evd_cross_kernel / quad_update_kernel); the apply is a persistent grid.
static void quad_geometry(Geometry& g, int P, int m_pad, int n_v) {
  // gram_quad_kernel: one workgroup (160 KB LDS, one per CU) per quad and row
  // chunk, ~256 of them; from 32 quads per launch every quad keeps 4 chunks,
  // so a merged one-GPU launch (two chains' quads in one) sums every Gram
  // exactly as the two chains do (bitwise the same solve, as make_geometry).
  // 64 quads (16384^2 merged), us per quad step: 2 chunks 963-979, 4 chunks
  // 874-884, 8 chunks 933 (profiles/r5_gram)
  const int nq = P / 2 > 0 ? P / 2 : 1;
  int want = nq >= 32 ? 4 : (256 + nq - 1) / nq;
  static const int forced = svdj_debug_knob("quad_gram_chunks", 0);  // A/B only (svdj_debug.h)
  if (forced > 0) want = forced;
  const int maxc = m_pad / 128;
  g.qgch = want < 1 ? 1 : (want > maxc ? maxc : want);
  g.qgrows = round_up((m_pad + g.qgch - 1) / g.qgch, 128);
  g.qgch = (m_pad + g.qgrows - 1) / g.qgrows;
}

static Geometry make_geometry(int W, int P, int m_pad, int n_v, int mma = 0) {
  Geometry g;
  // Gram: split-K over row chunks (>= 128 rows each), ~512 workgroups.
  // Many pairs per step want few chunks (every chunk is a slab the EVD sums:
  // 1-GPU 16384^2, W=64, 5.92 s at 512 vs 6.23 s at 2048).  With few pairs
  // (many GPUs) 64-256 measured slower (8-GPU rank plan 65.5 -> 74-78 ms).
  // With the split-bf16 apply, steps of >= 32 pairs want ~256 (1 GPU 16384^2
  // 4.94 -> 4.84 s, 8192^2 674 -> 659 ms, P=2 plan 165.8 -> 163.5 ms per sweep);
  // the P=4 plan (16 pairs) is 6 % slower at 256 (profiles/r3_s3/gram).
  // Steps of >= 64 pairs keep the 64-pair chunking (4 row chunks): a merged
  // one-GPU step (two chains' 64-pair steps in one launch, pipeline.py
  // run_merged) then sums every pair's Gram exactly as the two chains do, so
  // the solve is bitwise the two-chain one (same sweeps).  Measured at 128
  // pairs (16384^2 merged, quad off): 4 chunks 4.70 s vs 2 chunks (the
  // target rule) 4.73 s, residual 1.37e-5 vs 1.52e-5 (profiles/r5_gram).
  // Round 5 (profiles/r5_ab): below 32 pairs, at most ~512 workgroups AND
  // chunks of at least 512 rows -- rank plans, ms per sweep: 16384^2 P = 8
  // (8 pairs) 53.5 at 256 rows (512 workgroups, the old rule), 52.9 at 384,
  // 43.5 at 512, 55.2 at 1024; P = 4 (16 pairs) 100.9 / 82.8 / 83.9 / 86.7 at
  // 256 / 384 / 512 / 1024 rows; 32768 x 32768 P = 8 (16 pairs) 307 at 1024
  // rows (512 workgroups) vs 325 at 512 (1024 workgroups).  The EVD sums one
  // slab per chunk, so short chunks put more slab data on its critical path.
  int want = P >= 32 ? (256 + P - 1) / P : min((m_pad + 511) / 512, (512 + P - 1) / P);
  // (the bump applies to the split-bf16 launches it was measured on: merged
  // fp32 one-GPU steps of 128 pairs; fp64 steps keep the target rule)
  if (mma != 0 && P >= 64 && want < 4) want = 4;
  static const int forced = svdj_debug_knob("gram_chunks", 0);  // A/B only (svdj_debug.h)
  if (forced > 0) want = forced;
  int maxc = m_pad / 128;
  g.gchunks = want < 1 ? 1 : (want > maxc ? maxc : want);
  g.grows = round_up((m_pad + g.gchunks - 1) / g.gchunks, 128);
  g.gchunks = (m_pad + g.grows - 1) / g.grows;
  // Apply: workgroups over A and V rows (128..2048 rows each, every one
  // fills the pair's 2W x 2W Q into LDS first).  ~2048 workgroups for W = 32
  // and for steps with >= 64 pairs (one GPU: 16384^2 5.79 s vs 5.87 s at
  // 512); ~512 for W = 64 with fewer pairs, where the 64 KB Q fill of short
  // workgroups costs more than the occupancy gains: 16384^2 rank plans
  // P=2/4/8 206.5/126.2/63.0 -> 203.5/114.5/59.8 ms per sweep, 8192^2 one GPU
  // 866 -> 799 ms, 32768x8192 (QR) 943 -> 888 ms; W = 32 (4096^2, fp64
  // 5000^2) 2-3.5 % slower at 512 (profiles/r2_awg).  The split-bf16 applies
  // (mma != 0) keep 2048: their larger Q images (32768x8192 bf16 with QR:
  // 811 -> 847 ms at 512).
  int total_rows = m_pad + n_v;
  // The split-bf16 apply (mma != 0, Q held in registers per output column
  // tile) wants 2048 unless a step has few pairs: 1 GPU 8192^2 664 ms at
  // 2048 vs 756 at 512, 16384^2 P=8 rank plan 52.3 vs 50.3 ms per sweep at
  // 2048 vs 512 (profiles/r3_s3/bf16x6).
  const int wg_target = mma == 0 ? (W == 64 && P < 64 ? 512 : 2048) : (P <= 16 ? 512 : 2048);
  int rows = round_up((int)(((long)total_rows * P + wg_target - 1) / wg_target), 128);
  if (rows < 128) rows = 128;
  if (rows > 2048) rows = 2048;
  g.rows_a = rows;
  g.rows_v = rows;
  g.a_chunks = (m_pad + rows - 1) / rows;
  g.v_chunks = n_v > 0 ? (n_v + rows - 1) / rows : 0;
  quad_geometry(g, P, m_pad, n_v);
  return g;
}

static bool has_quad(int esize, int W) { return esize == 4 && W == 64; }
// Mode (SVDJ_STEP_*, svdj_hip.h) of step s of a mode list; no list: all cross.
static int step_mode(const int32_t* modes, int s) { return modes ? modes[s] : SVDJ_STEP_CROSS; }
static bool has_quad_steps(const int32_t* modes, int steps) {
  for (int s = 0; modes && s < steps; ++s)
    if (modes[s] == SVDJ_STEP_QUAD) return true;
  return false;
}

// One chain of steps: resident buffers, its pair list, the parameters of its
// steps and its workspace.
template <typename T>
struct Chain {
  int m_pad, lda, n_v, ldv, P, steps;
  T *A, *V, *D;
  const int32_t* pairs;
  const int32_t* modes;
  double tol;  // the EVDs' rotation threshold, relative or (tol_mode 1) absolute
  int tol_mode, max_inner;
  uint32_t* metric;  // svdj_stop.h
  // 0: one metric.  g > 0: metric is uint32[groups][SVDJ_METRIC_WORDS] and a
  // pair (bi, bj) accumulates into group bi / g (svdj_block_steps_grouped)
  int group_blocks;
  int mma;  // the apply's matrix-core mode (SVDJ_MMA_*)
  int gram_np;  // bf16 parts of the quad Gram (3; 2: SVDJ_STEPS_GRAM2)
  int shared;  // another chain runs concurrently on this GPU (SVDJ_STEPS_SHARED_GPU)
  Geometry g;
  T* slabs;
  T* xsum;  // cross slabs summed over their row chunks, inside the slab area (launch_evd)
  T* Qb[2];
  int32_t* skipb[2];
  T* rec;  // cross EVD rotation records (tangents)
  int32_t* nsteps;
  // quad steps (has_quad)
  float* qslabs;
  float* qred;  // the 3P Grams summed over their row chunks (when qgch > 4)
  double* T1;
  float* upd;
  bf16x8* Ts[2];
  int32_t* skip1[2];
  int32_t* skip2[2];
  hipStream_t st;
};

// Workspace areas in the order they are taken, each rounded up to 256 bytes.
// With a null base nothing is handed out and `off` ends as the byte count,
// so one layout routine gives a workspace's size and its carve-up.
static size_t rup256(size_t b) { return (b + 255) / 256 * 256; }
struct Bump {
  char* base;
  size_t off;
  template <typename T>
  T* take(size_t bytes) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += rup256(bytes);
    return p;
  }
};

// The layout routines below read c.P and the chunk counts in c.g, set the
// chain's workspace pointers (null for a null ws) and return the byte count.

// c.g.gchunks full-Gram (2W x 2W) slabs per pair; cross slabs (W x W) fill
// the first quarter, and their sums over the chunks (launch_evd) follow them.
template <typename T>
static void take_slabs(Chain<T>& c, Bump& b, int W) {
  c.slabs = b.take<T>((size_t)c.P * c.g.gchunks * 4 * W * W * sizeof(T));
  c.xsum = c.slabs ? c.slabs + (size_t)c.P * c.g.gchunks * W * W : nullptr;
}
// The cross EVD's rotation records and step counts (consumed by qbuild(s)
// before evd(s+1) on the same stream: single-buffered).
template <typename T>
static void take_records(Chain<T>& c, Bump& b, int W) {
  c.rec = b.take<T>((size_t)c.P * kCrossMaxInner * W * W * sizeof(T));
  c.nsteps = b.take<int32_t>((size_t)c.P * sizeof(int32_t));
}

// A solve's workspace: slabs, double-buffered Q and skip flags (evd(s+1) may
// run while apply(s) reads), records.  With quad steps (fp32 W = 64) also the
// 3P quad Gram slabs and their chunk sums, T1 (fp64 Q of the P step-s pairs),
// the step-(s+1) couplings, the double-buffered split T - I (P/2 quads x 256
// x 256 in 3 bf16 parts = 1.5 x an fp32 T each) and both EVDs' skip flags.
template <typename T>
static size_t solve_layout(Chain<T>& c, void* ws, int W, bool quad) {
  Bump b{(char*)ws, 0};
  const size_t P = c.P, flags = P * sizeof(int32_t);
  take_slabs(c, b, W);
  for (T*& q : c.Qb) q = b.take<T>(P * 4 * W * W * sizeof(T));
  for (int32_t*& k : c.skipb) k = b.take<int32_t>(flags);
  take_records(c, b, W);
  if (quad && has_quad(sizeof(T), W)) {
    c.qslabs = b.take<float>(3 * P * c.g.qgch * W * W * sizeof(float));
    c.qred = b.take<float>(3 * P * W * W * sizeof(float));
    c.T1 = b.take<double>(P * 4 * W * W * sizeof(double));
    c.upd = b.take<float>(P * W * W * sizeof(float));
    const size_t tstride = rup256((size_t)(c.P / 2 > 0 ? c.P / 2 : 1) * 16 * W * W * sizeof(float));
    c.Ts[0] = b.take<bf16x8>(3 * tstride);  // 3 bf16 parts = 1.5 x the fp32 size of T
    c.Ts[1] = c.Ts[0] ? (bf16x8*)((char*)c.Ts[0] + 3 * tstride / 2) : nullptr;
    for (int32_t*& k : c.skip1) k = b.take<int32_t>(flags);
    for (int32_t*& k : c.skip2) k = b.take<int32_t>(flags);
  }
  return b.off;
}
// svdj_evd_alone's: the slab area of a step with c.g.gchunks chunks, records.
template <typename T>
static size_t evd_alone_layout(Chain<T>& c, void* ws, int W) {
  Bump b{(char*)ws, 0};
  take_slabs(c, b, W);
  take_records(c, b, W);
  return b.off;
}
template <typename T>
static size_t evd_alone_ws_bytes(int W, int P, int nchunk) {
  Chain<T> c{};
  c.P = P;
  c.g.gchunks = nchunk;
  return evd_alone_layout(c, nullptr, W);
}
// svdj_quad_chain's: the chunk sums of the 3P quad Grams, records.
static size_t quad_chain_layout(Chain<float>& c, void* ws) {
  Bump b{(char*)ws, 0};
  c.qred = b.take<float>((size_t)3 * c.P * 64 * 64 * sizeof(float));
  take_records(c, b, 64);
  return b.off;
}

// Bytes of a solve's workspace.  The Gram chunking depends on the apply mode
// (split-bf16 launches may take more chunks): the slabs are sized for the
// larger of the two, whichever chain_init then carves.
template <typename T>
static size_t solve_ws_bytes(int W, int P, int m_pad, bool quad) {
  Chain<T> c{};
  c.P = P;
  c.g = make_geometry(W, P, m_pad, 0, 0);
  const Geometry gs = make_geometry(W, P, m_pad, 0, 1);
  if (gs.gchunks > c.g.gchunks) c.g = gs;
  return solve_layout(c, nullptr, W, quad);
}

}  // namespace svdj
