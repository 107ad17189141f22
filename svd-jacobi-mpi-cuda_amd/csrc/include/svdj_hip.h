// Device-side (MI355X / gfx950) native API of the Jacobi-SVD framework.
//
// Plain C ABI over raw device pointers + a hipStream_t passed as void*, so the
// library has no PyTorch dependency: Python binds it with ctypes and passes
// tensor.data_ptr() / torch.cuda.current_stream().cuda_stream; the native C++
// driver links it directly.
//
// Storage convention (all entry points): a column-major matrix with leading
// dimension ld is addressed as column c at base + c*ld.  Row counts passed to
// kernels are PADDED row counts (multiple of SVDJ_ROW_ALIGN, pad rows zero),
// so no kernel needs a row bounds check.
//
// dtype codes: 0 = fp32, 1 = fp64.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define SVDJ_ROW_ALIGN 128
#include "svdj_stop.h"

#ifdef __cplusplus
extern "C" {
#endif

// Returns a static version/feature string ("gfx950 ...").
const char* svdj_hip_version(void);
// Last error message recorded by this library (thread-local), "" if none.
const char* svdj_hip_last_error(void);

// ---------------------------------------------------------------------------
// Scalar (column-pair) path: one fused kernel per parallel step, one
// workgroup per pair (wave64 reductions of the reference's dot triple,
// rotation solved in registers, Givens update of A and V in place).
//   sched     device int32 [steps][per_step][2] (pairs < 0 are skipped)
//   tol_mode  0 relative, 1 absolute
//   metric    device uint32[2]: [0] = max convergence value (float bits),
//             [1] = number of rotations applied.  Accumulated (not reset).
int svdj_scalar_step(int dtype, int m_pad, void* A, int lda, void* V, int n_v,
                     int ldv, const int32_t* sched, int per_step, double tol,
                     int tol_mode, uint32_t* metric, void* stream);

// Full solve on one GPU: repeats sweeps over `steps` until a sweep applies
// no rotation or max_sweeps is reached.  hist (host, may be NULL) receives
// the per-sweep max convergence value.  Returns sweeps executed, <0 on error.
int svdj_scalar_solve(int dtype, int m_pad, void* A, int lda, void* V, int n_v,
                      int ldv, const int32_t* sched, int steps, int per_step,
                      double tol, int tol_mode, int max_sweeps, uint32_t* metric,
                      double* hist, void* stream);

// ---------------------------------------------------------------------------
// Block path (one-sided block Jacobi, MFMA).  Columns are grouped in blocks
// of W (32 or 64; fp64 supports 32).  One step processes P disjoint block
// pairs (bi, bj):
//   1. Gram (MFMA, split over rows):  cross C = A_bi^T A_bj,
//                                     full  G = [A_bi A_bj]^T[..]
//   2. EVD of the 2W x 2W Gram (cyclic parallel Jacobi in LDS), in cross
//      mode with the diagonal blocks taken from the tracked squared column
//      norms D (blocks are kept internally orthogonal);  Q -> workspace.
//   3. Apply (MFMA):  [A_bi A_bj] <- [A_bi A_bj] Q ,  [V_bi V_bj] <- .. Q
// D (device, dtype, [ncols]) holds squared column norms; updated in place.
//   pairs   device int32 [steps][P][2] block indices
//   modes   host   int32 [steps] of SVDJ_STEP_* (below), NULL = all
//           SVDJ_STEP_CROSS:
//             CROSS       cross Gram, cyclic EVD (2W-1 EVD steps)
//             FULL        full Gram, cyclic EVD
//             CROSS_BIP   cross Gram, bipartite EVD ordering (W EVD steps)
//             CROSS_ONLY  cross Gram, cross-only bipartite EVD + Q build
//             QUAD        first step of a quad (fp32, W = 64, a split-bf16
//                         mma): steps s and s+1 over the four blocks of every
//                         two consecutive pairs, (a,c),(b,d) then (a,d),(b,c),
//                         run fused -- six cross Grams, two cross EVDs, one
//                         apply.  Needs an even P and SVDJ_STEP_QUAD_SECOND
//                         as the mode of step s+1.
//             QUAD_SECOND second step of a quad: launches nothing (its
//                         first step did the work); only valid after QUAD.
//   metric  device uint32[SVDJ_METRIC_WORDS] (svdj_stop.h): [0] max
//           convergence value (float bits), [1] rotated pairs, [2..3] the
//           underflow floor (double, svdj_set_norm_floor; 0 = off), [4] the
//           largest |sin| of an applied rotation (float bits).
//   tol_mode 0: rotate when |g_pq| > tol sqrt(g_pp g_qq) (relative, default);
//            1: when |g_pq| > tol (the reference's absolute TOLERANCE test).
//   mma     a flags word.  mma & SVDJ_MMA_MASK is the apply's matrix-core
//           mode: SVDJ_MMA_NATIVE (f32 / f64 MFMA), SVDJ_MMA_BF16X6 (fp32 data
//           on bf16 MFMA, 3-way bf16 split: 6 products, fp32-level accuracy),
//           SVDJ_MMA_BF16X3 (2-way split: 3 products, ~2^-17).  Both split
//           modes apply Y = X + X (Q - I), the identity in fp32.  Or'ed in:
//             SVDJ_STEPS_GRAM2       the quad Gram of quad steps on 2 bf16
//                                    parts (3 products, couplings to ~2^-17)
//                                    -- for sweeps far from convergence, where
//                                    it only steers the rotation angles;
//             SVDJ_STEPS_SHARED_GPU  another chain runs concurrently on this
//                                    GPU: the quad apply leaves it a share of
//                                    the CUs (a smaller persistent grid).
enum {
  SVDJ_STEP_CROSS = 0,
  SVDJ_STEP_FULL = 1,
  SVDJ_STEP_CROSS_BIP = 2,
  SVDJ_STEP_CROSS_ONLY = 3,
  SVDJ_STEP_QUAD = 4,
  SVDJ_STEP_QUAD_SECOND = 5
};
enum { SVDJ_MMA_NATIVE = 0, SVDJ_MMA_BF16X6 = 1, SVDJ_MMA_BF16X3 = 2 };
enum { SVDJ_MMA_MASK = 0xff, SVDJ_STEPS_GRAM2 = 0x100, SVDJ_STEPS_SHARED_GPU = 0x200 };
// bf16 parts of a matrix-core mode's operand split; 0: native, no split.
static inline int svdj_mma_parts(int mma) {
  return mma == SVDJ_MMA_BF16X6 ? 3 : mma == SVDJ_MMA_BF16X3 ? 2 : 0;
}
// inner_order codes of svdj_block_solve / svdj_dist_problem: the EVD of the
// cross steps (SVDJ_STEP_CROSS / CROSS_BIP / CROSS_ONLY); AUTO resolves by
// svdj_choose_inner_order.
enum {
  SVDJ_INNER_CYCLIC = 0,
  SVDJ_INNER_BIPARTITE = 1,
  SVDJ_INNER_CROSS = 2,
  SVDJ_INNER_AUTO = 3
};
// The cross steps' mode for a resolved inner_order (not AUTO).
static inline int svdj_cross_step_mode(int inner_order) {
  return inner_order == SVDJ_INNER_CROSS    ? SVDJ_STEP_CROSS_ONLY
         : inner_order == SVDJ_INNER_CYCLIC ? SVDJ_STEP_CROSS
                                            : SVDJ_STEP_CROSS_BIP;
}
// Workspace size for steps of P pairs: svdj_block_workspace_bytes(); quad != 0
// when the step list holds quad steps.
size_t svdj_block_workspace_bytes(int dtype, int W, int P, int m_pad, int quad);
// inner_order code (SVDJ_INNER_BIPARTITE or SVDJ_INNER_CROSS) for steps of
// `pairs` pairs of W-wide blocks of data type `dtype` (0 fp32, 1 fp64):
// models/block.py choose_inner_order.
int svdj_choose_inner_order(int dtype, int W, int pairs);
// Default ("auto") matrix-core mode for dtype (0 fp32, 1 fp64) and block width
// W: SVDJ_MMA_BF16X6 for fp32 W = 64, else SVDJ_MMA_NATIVE (models/block.py
// choose_mma).
int svdj_choose_mma(int dtype, int W);
int svdj_block_steps(int dtype, int W, int m_pad, void* A, int lda, void* V,
                     int n_v, int ldv, void* D, const int32_t* pairs, int P,
                     int steps, const int32_t* modes, double tol, int tol_mode,
                     int max_inner_sweeps, void* workspace, size_t ws_bytes,
                     uint32_t* metric, int mma, void* stream);
// svdj_block_steps with one metric per group of blocks: metric is device
// uint32[groups][SVDJ_METRIC_WORDS], and a pair (bi, bj) reads the floor of and
// accumulates into group bi / group_blocks (group_blocks > 0; both blocks of a
// pair must lie in one group).  With B matrices stacked side by side as column
// blocks of one array, k blocks each, group_blocks = k makes a step whose pair
// list never crosses a matrix B independent block-Jacobi steps in one launch,
// each with its own stop-test words.  group_blocks = 0 is svdj_block_steps.
// Quad modes are refused (-2) when group_blocks != 0.
int svdj_block_steps_grouped(int dtype, int W, int m_pad, void* A, int lda, void* V, int n_v,
                             int ldv, void* D, const int32_t* pairs, int P, int steps,
                             const int32_t* modes, double tol, int tol_mode,
                             int max_inner_sweeps, void* workspace, size_t ws_bytes,
                             uint32_t* metric, int group_blocks, int mma, void* stream);

// Single-GPU block solve: round-robin over nb = ncols/W blocks (nb even),
// first step of every sweep SVDJ_STEP_FULL; inner_order (SVDJ_INNER_*) gives
// the other steps' mode: CYCLIC SVDJ_STEP_CROSS, BIPARTITE SVDJ_STEP_CROSS_BIP,
// CROSS SVDJ_STEP_CROSS_ONLY, AUTO by svdj_choose_inner_order.  stop_rule 1: a
// sweep also ends the iteration by the second-order rule of svdj_stop.h
// (relative mode), 0: only a sweep without rotations does.  Returns sweeps,
// <0 on error.
int svdj_block_solve(int dtype, int W, int m_pad, void* A, int lda, void* V,
                     int n_v, int ldv, void* D, int ncols, double tol, int tol_mode,
                     int max_inner_sweeps, int max_sweeps, int inner_order, void* workspace,
                     size_t ws_bytes, uint32_t* metric, double* hist,
                     int mma, int stop_rule, void* stream);
// Zero the per-sweep words of a block-path metric ([0], [1], [4..7]); the
// floor ([2..3]) stays.
int svdj_reset_metric(uint32_t* metric, void* stream);

// Diagnostic hooks.  Each runs one stage of a step through the launcher a
// solve calls for it (block_launch.hpp launch_*), on buffers given by the caller.
// The Gram of one step for a device pair list with the given row chunking
// (rows_per_chunk a multiple of SVDJ_ROW_ALIGN; chunk c = rows [c rows,
// min(m_pad, (c + 1) rows))), unsummed: mode SVDJ_STEP_CROSS slabs (P x nchunk
// x W x W) of A_bi^T A_bj, SVDJ_STEP_FULL (P x nchunk x 2W x 2W) of
// [A_bi A_bj]^T [A_bi A_bj].  fp32 and fp64, W = 32 and 64 (fp32 W = 64: lda a
// multiple of 4).
int svdj_gram(int dtype, int W, int mode, const void* A, int lda, int m_pad,
              const int32_t* pairs, int P, int rows_per_chunk, void* slabs, void* stream);
// svdj_gram with SVDJ_STEP_CROSS.
int svdj_gram_cross(int dtype, int W, const void* A, int lda, int m_pad,
                    const int32_t* pairs, int P, int rows_per_chunk, void* slabs, void* stream);
// The six cross Grams of a quad step (fp32, W = 64; pairs in quad order,
// P even): slabs (3P x nchunk x W x W) = the P pairs' Grams, then C_ad, C_bc,
// C_ab, C_cd of every quad.  parts: 3 (exact to 2^-26) or 2 (2^-16, the
// early-sweep Gram of svdj_block_steps' SVDJ_STEPS_GRAM2).
int svdj_gram_quad(const void* A, int lda, int m_pad, const int32_t* pairs, int P,
                   int rows_per_chunk, void* slabs, int parts, void* stream);
// X <- X Q for one pair of column blocks (X = 2W columns, leading dimension
// ld, `rows` a multiple of SVDJ_ROW_ALIGN), Q row-major 2W x 2W on the
// device, with matrix-core mode `mma` (as svdj_block_steps).
int svdj_apply_q(int dtype, int W, int mma, void* X, int rows, int ld, const void* Q, void* stream);
// The quad step's apply alone (fp32, W = 64): [a b c d] <- [a b c d] T in
// place on A (m_pad rows) and V (n_v rows; NULL: A only) for each of the nq
// quads, launched as a quad step of svdj_block_steps launches it.
//   pairs   device int32 [2 nq][2], quad order: (a,c), (b,d) per quad
//   Ts      device bf16: T - I of every quad (T rounded to fp32 first) split
//           into np round-to-nearest-even bf16 parts, part p of
//           (T - I)[32 kb + 8 g + e][32 ct + 16 cs + i] at
//           [q][kb][ct][cs][p][lane = 16 g + i][e]  (q < nq; kb, ct < 8; cs < 2;
//           g < 4; i < 16; e < 8)
//   skip1, skip2  device int32 [2 nq] each: quad q is skipped (its columns
//           untouched, its Ts never read) when its four flags are all nonzero
//   np      2 or 3 parts (svdj_mma_parts of svdj_block_steps' mma)
//   grid    workgroups of the persistent kernel, >= 1 (256; 192 / 224 next to
//           a second chain)
//   cheap_log2  np = 3: a 128-row half of a 32-column tile of T - I whose
//           largest part 0 is <= 2^-cheap_log2 takes the first-order form
//           (production: 7; 126: never)
//   work    device uint32[2] or NULL, accumulated: [0] MFMAs issued / 24,
//           [1] 32-row tiles moved (metric words 6, 7 of svdj_stop.h)
// lda, ldv multiples of 4.  Returns < 0 with the error string set, nothing
// launched, on a bad argument.
int svdj_apply_quad(void* A, int lda, int m_pad, void* V, int n_v, int ldv, const int32_t* pairs,
                    int nq, const void* Ts, const int32_t* skip1, const int32_t* skip2, int np,
                    int grid, int cheap_log2, uint32_t* work, void* stream);
// The middle of a single step alone: everything a step of svdj_block_steps
// runs after its Gram (mode SVDJ_STEP_CROSS to SVDJ_STEP_CROSS_ONLY; the
// variants of CROSS_ONLY's chunk pre-sum and Q build selected by P and nchunk
// as in a solve), from Gram slabs given by the caller.
//   slabs   device, data type: P x nchunk x W x W (SVDJ_STEP_FULL: 2W x 2W),
//           summed over the nchunk chunks by the kernels
//   D       device, squared column norms by block id; updated in place
//   pairs   device int32 [P][2]; metric: device uint32[8] (svdj_stop.h),
//           floor set
//   Q       out, P x 2W x 2W row-major (a skipped pair's is not written)
//   skip    out, int32 [P]
//   ws      device, svdj_evd_alone_workspace_bytes(dtype, W, P, nchunk) bytes
// Returns -2 with the error string set, nothing launched, on a bad argument.
size_t svdj_evd_alone_workspace_bytes(int dtype, int W, int P, int nchunk);
int svdj_evd_alone(int dtype, int W, int mode, const void* slabs, int nchunk, void* D,
                   const int32_t* pairs, int P, double tol, int tol_mode, int max_inner, void* Q,
                   int32_t* skip, void* ws, size_t ws_bytes, uint32_t* metric, void* stream);
// The middle of a quad step alone (fp32, W = 64): everything a quad step runs
// between its Gram and its apply (chunk pre-sum, EVD 1, T1, Gram-space update,
// EVD 2, split T; variants selected by P and nchunk as in a solve).
//   slabs   device fp32, 3P x nchunk x 64 x 64 in svdj_gram_quad's order
//   pairs   device int32 [2][P][2]: quad order (a,c), (b,d), then (a,d), (b,c)
//   np      2 or 3 parts of the split T
//   T1      out, fp64 P x 128 x 128 (identity for a pair EVD 1 skipped)
//   upd     out, fp32 P x 64 x 64: the couplings EVD 2 reads
//   Ts      out, bf16 (P / 2) x 256 x 256 x np in svdj_apply_quad's layout
//   skip1, skip2  out, int32 [P] each
//   ws      device, svdj_quad_chain_workspace_bytes(P) bytes
// Returns -2 with the error string set, nothing launched, on a bad argument
// (odd P included).
size_t svdj_quad_chain_workspace_bytes(int P);
int svdj_quad_chain(const void* slabs, int nchunk, void* D, const int32_t* pairs, int P, double tol,
                    int tol_mode, int max_inner, int np, void* T1, void* upd, void* Ts,
                    int32_t* skip1, int32_t* skip2, void* ws, size_t ws_bytes, uint32_t* metric,
                    void* stream);

// ---------------------------------------------------------------------------
// Batched path (csrc/hip/batched.hip): `batch` independent small SVDs in one
// launch, one workgroup per matrix, the matrix and V resident in LDS from
// load to store (scalar one-sided Jacobi, round-robin ordering, the scalar
// path's rotation test with the block path's underflow floor per matrix,
// sigma / U finalize fused).  Envelope: m >= n, 1 <= n <= 64, and
// svdj_batched_lds_bytes(dtype, m, n, V != NULL) != 0.
//
// The LDS bytes a workgroup takes for an (m x n) matrix, from the layout
// routine the kernel carves its LDS with; 0: outside the envelope or above
// the 163840-byte cap (a CU's whole LDS).
size_t svdj_batched_lds_bytes(int dtype, int m, int n, int want_v);
// Threads of the workgroup that solves a matrix of n columns (8 lanes per
// column pair of a step, rounded up to whole waves); 0 for n outside [1, 64].
int svdj_batched_threads(int n);
// The solve:
//   A       device, read in place through element strides: matrix b, row i,
//           column j at A[b sb + i sr + j sc] (loads are coalesced when sc or
//           sr is 1: a contiguous (batch, m, n) tensor, or the transposed
//           view of a contiguous (batch, n, m) one)
//   U       out, contiguous (batch, m, n) row-major, or NULL: not computed
//   S       out, contiguous (batch, n), unsorted
//   V       out, contiguous (batch, n, n) row-major (V, not V^T), or NULL:
//           not accumulated and no LDS taken for it
//   tol, tol_mode  as svdj_scalar_step (the absolute test is on the caller's
//           matrix, whatever the kernel's internal scaling); in both modes a
//           pair with a squared norm at or below the underflow floor is not
//           rotated; a matrix stops after a sweep that rotated nothing, or
//           after max_sweeps sweeps
//   sweeps  out, device int32 [batch]: sweeps run per matrix
//   off     out, device float [batch]: largest |a_p.a_q| / (|a_p| |a_q|) seen
//           in the matrix's last sweep
// Returns 0; -2 with the error string set and nothing launched on a bad
// argument (bad dtype, m < n, n > 64, does not fit in LDS, max_sweeps < 0,
// NULL A / S / sweeps / off); batch == 0 returns 0 without any HIP call.
int svdj_batched_svd(int dtype, int batch, int m, int n, const void* A, long sb, long sr,
                     long sc, void* U, void* S, void* V, double tol, int tol_mode,
                     int max_sweeps, int32_t* sweeps, float* off, void* stream);

// ---------------------------------------------------------------------------
// Batched path for tall matrices (csrc/hip/batched_tall.hip): any m >= n with
// 1 <= n <= 64 and m n < 2^31, one workgroup of 256 threads per matrix.  The
// workgroup streams A through LDS in panels of `panel_rows` rows, folds each
// into a resident n x n R with Householder reflectors (flat-tree TSQR), runs
// the batched path's Jacobi on R with V, and streams back through the panels
// to form U = Q U_R.  R and V always fit, so no row count is refused.
//
// The LDS bytes a workgroup takes at n columns and panels of panel_rows rows
// (a positive multiple of 8), from the layout routine the kernel carves its
// LDS with: R image, V image (want_v), two panel images, three per-reflector
// slot arrays, sigma, scratch; 0: bad arguments or above the 163840-byte cap.
size_t svdj_batched_tall_lds_bytes(int dtype, int n, int want_v, int panel_rows);
// The panel height svdj_batched_tall_svd takes for panel_rows = 0: the largest
// multiple of 8 that fits in half a CU's LDS (two workgroups per CU) if that
// is at least 64 rows, else the largest that fits in all of it.
int svdj_batched_tall_panel_rows(int dtype, int n, int want_v);
// The solve.  A, S, V, tol, tol_mode, max_sweeps, sweeps, off: as
// svdj_batched_svd (sweeps and off are those of the Jacobi on R).
//   U       out, contiguous (batch, m, n) row-major, or NULL: not computed.
//           Between the QR and the U stage it holds the reflector vectors.
//   tau_ws  device workspace of batch x ceil(m / panel_rows) x n elements of
//           the data type (the reflectors' taus); needed when U is not NULL
//   panel_rows  0: svdj_batched_tall_panel_rows; else a positive multiple of 8
// Returns 0; -2 with the error string set and nothing launched on a bad
// argument (bad dtype, m < n, n > 64, m n >= 2^31, panel_rows negative, not a
// multiple of 8 or too large for LDS, max_sweeps < 0, NULL A / S / sweeps /
// off, U without tau_ws); batch == 0 returns 0 without any HIP call.
int svdj_batched_tall_svd(int dtype, int batch, int m, int n, const void* A, long sb, long sr,
                          long sc, void* U, void* S, void* V, void* tau_ws, int panel_rows,
                          double tol, int tol_mode, int max_sweeps, int32_t* sweeps, float* off,
                          void* stream);

// ---------------------------------------------------------------------------
// Batched path for matrices wider than 64 columns (csrc/hip/batched_block.hip):
// the pack and finalize passes around svdj_block_steps_grouped.  `batch`
// matrices (m x n, m >= n >= 1) are stacked side by side in one column-major
// image At of m_pad rows (a multiple of SVDJ_ROW_ALIGN, >= m) and batch x
// ncols columns (ncols a multiple of 64, >= n): matrix b's column j is stacked
// column b ncols + j; pad rows and columns are zero.  The stacked V has n_v
// rows (a multiple of SVDJ_ROW_ALIGN, >= ncols).  At most 65535 matrices and
// 2^31 - 1 stacked columns per call.
//
// Pack: reads A once through element strides (sb, sr, sc) as svdj_batched_svd
// does (coalesced when sc or sr is 1) and writes
//   At      the stacked image
//   V       NULL, or the stacked V: an identity block per matrix
//   D       [batch ncols], data type: squared column norms, fp64 accumulation
//   metric  uint32[batch][SVDJ_METRIC_WORDS]: matrix b's underflow floor
//           max(m_pad realmin, m_pad realmin / eps * its largest D) in words
//           2..3 of its group, every other word zero
// Returns 0; -2 with the error string set and nothing launched on a bad
// argument; batch == 0 returns 0 without any HIP call.
int svdj_stack_pack(int dtype, int batch, int m, int n, const void* A, long sb, long sr, long sc,
                    int m_pad, int ncols, void* At, int lda, void* V, int n_v, int ldv, void* D,
                    uint32_t* metric, void* stream);
// Finalize: reads the stacked images once and writes
//   S       contiguous (batch, n): sigma = the fp64 column norm
//   U       NULL, or contiguous (batch, m, n) row-major: the columns of At,
//           divided by sigma when scale_u (a sigma == 0 column is left as it is)
//   Vout    NULL, or contiguous (batch, n, n) row-major from the stacked V
// Returns as svdj_stack_pack.
int svdj_stack_finalize(int dtype, int batch, int m, int n, int m_pad, int ncols, const void* At,
                        int lda, const void* V, int n_v, int ldv, void* U, void* S, void* Vout,
                        int scale_u, void* stream);

// ---------------------------------------------------------------------------
// Post-processing / utilities.
// V := I on an (n_v x ncols) column-major block (rows >= ncols zeroed).
int svdj_set_identity(int dtype, void* V, int n_v, int ldv, int ncols, int col_offset, void* stream);
// Squared column norms D[c] = sum_i A[i,c]^2 (fp64 accumulation).
int svdj_col_norms2(int dtype, const void* A, int m_pad, int lda, int ncols, void* D, void* stream);
// The block EVDs' underflow floor (relative mode: pairs with a squared norm
// <= it are not rotated): svdj_norm_floor_value = m realmin / eps of the
// data type; svdj_set_norm_floor stores it at metric[2..3] (metric holds 4
// uint32), once per solve.
double svdj_norm_floor_value(int dtype, int m);
int svdj_set_norm_floor(double floor, uint32_t* metric, void* stream);
// Scale-relative floor max(m realmin, m realmin / eps * max D) from the n squared
// column norms D (device, data type) into metric[2..3].
int svdj_set_norm_floor_scaled(int dtype, int m, const void* D, int n, uint32_t* metric,
                               void* stream);
// sigma[c] = ||a_c||; if scale_u, a_c /= sigma[c] (sigma == 0 columns untouched).
int svdj_finalize(int dtype, void* A, int m_pad, int lda, int ncols, void* sigma, int scale_u, void* stream);

// Device-side timed wait of `ns` nanoseconds on `stream` (one lane polling
// the constant 100 MHz clock); used to model link time in simulations.
int svdj_spin_ns(double ns, void* stream);

#ifdef __cplusplus
}
#endif
