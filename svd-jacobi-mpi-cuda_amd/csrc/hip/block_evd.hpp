// EVD stage of the block Jacobi step (block.hip) and the Q build: for the
// P block pairs (bi, bj) of a step,
//     evd   : G = [[D_bi, C], [C^T, D_bj]] -> Q^T G Q = Lambda by cyclic
//             parallel Jacobi held entirely in LDS (one 1024-thread WG per
//             pair); the convergence value max|g_pq|/sqrt(g_pp g_qq) of the
//             reference (main.cu:710) becomes the stop test;
#pragma once
#include "common.hpp"
#include "evd_deal_tables.hpp"
#include "svdj_stop.h"

namespace svdj {

// -------------------------------------------------------------------- evd
// The EVD of the 2W x 2W pair Gram runs in ONE workgroup per pair, as a
// cyclic parallel Jacobi (circle-method round robin: W disjoint rotations per
// step, 2W-1 steps per sweep):
//   * G lives in LDS in POSITION space (see pos_next below): every
//     off-diagonal slot-pair block (a < b) of a step is owned by one thread
//     for the whole kernel and its LDS addresses are static;
//   * ONE barrier per step.  The rotations of step st+1 are solved inside
//     step st's update phase: the coupling of a next-step pair lies in exactly
//     one off-diagonal block of step st, always the same one, so its owner
//     computes the new coupling, takes the post-step diagonals from the
//     step-st rotation records, solves step st+1's rotation right away and
//     publishes it (c, s, fp64 c/s and the post-rotation diagonals) into the
//     other half of a double-buffered record array.  The reference solves
//     every 2x2 on the host between two kernel launches (main.cu:698-725);
//   * the rotation accumulator Q lives in REGISTERS in fp64, in "slot layout":
//     lane (slot a, row group g) holds Q[k][first(a)] and Q[k][second(a)] for
//     its rows k.  The circle-method movement is a one-lane DPP shift per step
//     (wave_shr:1 / wave_shl:1); fp64 keeps Q orthogonal to ~1e-16 before it
//     is rounded to the data type, so V stays orthogonal over hundreds of
//     block steps;
//   * the diagonal never lives in G: it travels in the rotation records (a
//     rotation of slot a changes only d_first and d_second).
// Two values of one type, aligned to their combined size (one LDS access).
template <typename T>
struct alignas(2 * sizeof(T)) Pair2 {
  T x, y;
};

// Split-K slab loads in flight per thread while the EVD assembles G (with
// many GPUs a pair has up to 64 slabs of its Gram to sum, 1 MB for one
// workgroup).  8, 16 and 32 measured the same (8-GPU rank plan 59.5 / 60.0 /
// 59.9 ms per sweep): the slab sum is not what the EVD's latency is made of.
#define SVDJ_EVD_SLAB_UNROLL 8
constexpr int kEvdThreads = 1024;

// ------------------------------------------------------------ split-K slab sum
// A Gram arrives as nchunk slabs (one per row chunk of the data), `stride`
// elements apart.  THE sum of one 16-byte vector of them, at element `off` of
// the first slab: fp64 accumulators, chunk order, rounded once by the caller.
// Every consumer of slabs -- both EVD kernels, quad_update_kernel and
// slab_reduce_kernel -- sums with this function, so a pre-summed slab
// (slab_reduce_kernel, nchunk = 1 afterwards) is bitwise what the consumer
// would have summed from the chunks itself.  UNROLL: chunk loads in flight
// (#pragma unroll UNROLL; 0 leaves the loop to the compiler).
template <typename T, int N>
using vec = T __attribute__((ext_vector_type(N)));
template <int UNROLL, typename T>
__device__ __forceinline__ vec<double, 16 / (int)sizeof(T)> slab_sum(const T* base, int off,
                                                                    int stride, int nchunk) {
  constexpr int EV = 16 / (int)sizeof(T);
  vec<double, EV> acc = 0.0;
  auto add = [&](int k) {
    const auto v = *reinterpret_cast<const vec<T, EV>*>(base + (size_t)k * stride + off);
    acc += __builtin_convertvector(v, vec<double, EV>);
  };
  if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
    for (int k = 0; k < nchunk; ++k) add(k);
  } else {
    for (int k = 0; k < nchunk; ++k) add(k);
  }
  return acc;
}

// Slabs summed over their chunks ahead of their consumers, spread over many
// workgroups: with many chunks (few pairs per launch: 64 chunks at 4 quads)
// the latency-bound consumers, one workgroup per pair, then read one slab
// instead of all chunks (8-GPU plan: quad_update 334 us per launch reading 64
// chunks, profiles/r5_quad2).  W = 64, fp32: in = [slab][gch][W * W].
constexpr int kRedThreads = 256;
__global__ __launch_bounds__(kRedThreads) void slab_reduce_kernel(const float* __restrict__ in,
                                                                  int gch, float* __restrict__ out) {
  constexpr int W = 64;
  const int slab = blockIdx.x, e = 4 * (blockIdx.y * kRedThreads + threadIdx.x);
  const auto s = slab_sum<8>(in + (size_t)slab * gch * W * W, e, W * W, gch);
  *reinterpret_cast<f32x4*>(out + (size_t)slab * W * W + e) = __builtin_convertvector(s, f32x4);
}

// Lane i <- lane i-1 / i+1 across the wave (DPP wave_shr:1 / wave_shl:1).
// The edge lane receives 0 (bound_ctrl); every caller overwrites the edge
// slots by select, so no "old" value (and no register copy) is needed.
__device__ __forceinline__ int dpp_shr1(int v) {
  return __builtin_amdgcn_mov_dpp(v, 0x138, 0xf, 0xf, true);
}
__device__ __forceinline__ int dpp_shl1(int v) {
  return __builtin_amdgcn_mov_dpp(v, 0x130, 0xf, 0xf, true);
}
__device__ __forceinline__ float dpp_shr1(float v) {
  return __int_as_float(dpp_shr1(__float_as_int(v)));
}
__device__ __forceinline__ float dpp_shl1(float v) {
  return __int_as_float(dpp_shl1(__float_as_int(v)));
}
__device__ __forceinline__ double dpp_shr1(double v) {
  const long long x = __double_as_longlong(v);
  const int lo = dpp_shr1((int)(x & 0xffffffff)), hi = dpp_shr1((int)(x >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double dpp_shl1(double v) {
  const long long x = __double_as_longlong(v);
  const int lo = dpp_shl1((int)(x & 0xffffffff)), hi = dpp_shl1((int)(x >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Rotation test, shared by the solve and the "nothing to do" pre-pass so the
// two decide identically: relative |g_pq| > tol sqrt(g_pp g_qq) (fp32: raw
// v_sqrt, ~1 ulp), or the reference's absolute |g_pq| > tol (TOLERANCE,
// reference lib/global.cuh:9, main.cu:714) when absmode.
//
// Underflowing columns: in the relative mode a pair is rotated only if both
// squared norms exceed `floor` = m realmin / eps (metric[2..3], set once per
// solve, svdj_set_norm_floor).  Below it the squared norms and dot products
// of a column lose their precision to underflow (the entries' products
// approach realmin), so the relative coupling is noise and the pair would be
// rotated forever.  LAPACK's xGESVJ likewise skips columns below its safe
// minimum.  The reference's own input (upper-triangular U(0,1)) has
// sigma_min / sigma_max ~ 2^-n: at n = 5000 most columns end far below
// fp64's range, and without the floor the solve did not converge in 60
// sweeps (profiles/r3_refshape); columns above it keep one-sided Jacobi's
// relative accuracy (n = 300: U orthogonal to 1e-12).  0 = off.
__device__ __forceinline__ bool needs_rotation(float gpp, float gqq, float gpq, float tol,
                                               int absmode, float floor = 0.0f) {
  if (absmode) return fabsf(gpq) > tol;
  const float nrm = __builtin_amdgcn_sqrtf(gpp) * __builtin_amdgcn_sqrtf(gqq);
  return nrm > 0.0f && fabsf(gpq) > tol * nrm && fminf(gpp, gqq) > floor;
}
__device__ __forceinline__ bool needs_rotation(double gpp, double gqq, double gpq, double tol,
                                               int absmode, double floor = 0.0) {
  if (absmode) return fabs(gpq) > tol;
  const double nrm = sqrt(gpp) * sqrt(gqq);
  return nrm > 0.0 && fabs(gpq) > tol * nrm && fmin(gpp, gqq) > floor;
}
// Effective sine of a rotation for the second-order stop test
// (svdj_stop.h): |s| times the larger ratio of the two columns' norms after
// it (d = squared norms); 0 for no rotation.  Hardware rcp / sqrt (~1 ulp:
// a stop-test statistic; the IEEE division and square root were ~30
// instructions on the EVD solver lane's step).
template <typename T>
__device__ __forceinline__ float eff_sine(T s, T dp, T dq) {
  if (s == T(0)) return 0.0f;
  T pa = fabs(dp), pb = fabs(dq);
  if constexpr (sizeof(T) == 8) {
    // fp64 squared norms may lie outside float's range (a matrix scaled by
    // 2^200: the ratio became inf * 0 = NaN, atomic_max_pos dropped it, and
    // the second-order rule saw ms = 0 and stopped the solve after one sweep).
    // Bring the larger one to [0.5, 1) by a power of two first.  The scaling
    // itself is exact; a pair whose two squared norms were both normal floats
    // gives the value it gave as long as the smaller one stays a normal float
    // after the scaling, i.e. for ratios up to about 2^125.  Beyond that the
    // smaller one flushes to 0 and the result is the 1.0f cap below, where the
    // unscaled form gave a huge finite value or inf: either keeps the
    // second-order rule from firing.
    const int e = __builtin_amdgcn_frexp_exp(pa > pb ? pa : pb);
    pa = ldexp(pa, -e);
    pb = ldexp(pb, -e);
  }
  const float a = (float)pa, b = (float)pb;
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  return lo > 0.0f ? fabsf((float)s) * __builtin_amdgcn_sqrtf(hi * __builtin_amdgcn_rcpf(lo)) : 1.0f;
}
// The negligible-column floor of this solve (metric[2..3], a double).
template <typename T>
__device__ __forceinline__ T norm_floor(const uint32_t* metric) {
  return (T)*reinterpret_cast<const double*>(metric + 2);
}

// Rotation of one slot, branch-free (the solve sits on the EVD's critical
// path; the selects avoid exec-mask branches): c = 1, s = t = 0 when the
// test fails.  fp32: raw v_sqrt/v_rcp/v_rsq (~1 ulp) -- (c, s) only steer G;
// the fp64 Q is built from t.
__device__ __forceinline__ bool rotation_fast(float gpp, float gqq, float gpq, float tol,
                                              int absmode, float floor, float& c, float& s,
                                              float& t) {
  const bool rot = needs_rotation(gpp, gqq, gpq, tol, absmode, floor);
  // not `rot ? gpq : 1`: the rotation does not wait for the test (two
  // independent chains; a non-rotation is selected away below)
  const float g = gpq != 0.0f ? gpq : 1.0f;
  const float tau = (gqq - gpp) * __builtin_amdgcn_rcpf(2.0f * g);
  const float at = fabsf(tau);
  const float t_big = 0.5f * __builtin_amdgcn_rcpf(at);
  const float t_reg = __builtin_amdgcn_rcpf(at + __builtin_amdgcn_sqrtf(fmaf(tau, tau, 1.0f)));
  const float tt = at > 1e18f ? t_big : t_reg;
  t = rot ? (tau < 0.0f ? -tt : tt) : 0.0f;
  c = __builtin_amdgcn_rsqf(fmaf(t, t, 1.0f));
  s = t * c;
  return rot;
}
__device__ __forceinline__ bool rotation_fast(double gpp, double gqq, double gpq, double tol,
                                              int absmode, double floor, double& c, double& s,
                                              double& t) {
  const bool rot = needs_rotation(gpp, gqq, gpq, tol, absmode, floor);
  const double g = gpq != 0.0 ? gpq : 1.0;
  const double tau = (gqq - gpp) / (2.0 * g);
  const double at = fabs(tau);
  const double tt = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(fma(tau, tau, 1.0)));
  t = rot ? (tau < 0.0 ? -tt : tt) : 0.0;
  c = 1.0 / sqrt(fma(t, t, 1.0));
  s = t * c;
  return rot;
}
// fp64 1/sqrt(x) for x in [1, 2^60]: fp32 hardware estimate (~2^-22) and two
// Newton steps in fp64 (quadratic: 2^-44, then below fp64 rounding).
__device__ __forceinline__ double rsqrt64(double x) {
  double y = (double)__builtin_amdgcn_rsqf((float)x);
  const double hx = 0.5 * x;
  y = y * (1.5 - hx * y * y);
  y = y * (1.5 - hx * y * y);
  return y;
}

// Packed strict upper triangle of an N x N position-pair matrix.
template <int N>
__host__ __device__ constexpr int tri_idx(int i, int j) {
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a * N - a * (a + 1) / 2 + (b - a - 1);
}

// ---- inner orderings.  The kernel below is written against an ordering
// policy: where slot a's two players sit (first_pos / second_pos), how
// positions move per step (pos_next, prev_pos), which position pairs meet at
// the next step (next_meeting), the players of a slot at step st, and the
// register-Q movement (move).
//   EVD_CYCLIC: the circle-method round robin over all 2W players, 2W-1
//               steps per sweep (every pair of the 2W x 2W Gram);
//   EVD_BIP   : the bipartite ordering of the cross pairs only, W steps per
//               sweep: X players (block i) fixed at positions 0..W-1, the Y
//               player at Y-position p (position W+p) moves to p-1 (mod W);
//               slot a pairs positions (a, W+a).  Cross steps of a block
//               sweep use it (mode 2): the blocks' own columns are mutually
//               orthogonal when a cross step starts and the full-Gram step
//               at the start of every sweep rotates the within-block pairs,
//               so every column pair is still rotated once per sweep at half
//               the EVD steps (tests/test_schedule.py: bipartite data-flow
//               emulation; CPU block sweeps: same sweep count +-1).
enum { EVD_CYCLIC = 0, EVD_BIP = 1 };
template <int W, int ORD>
struct Ord;
// Position space.  The circle method fixes WHERE things happen and moves the
// players: ring positions 0..R-1 (R = 2W-1) plus the fixed position R of
// player N-1; slot a >= 1 owns positions (a-1, 2W-2-a), slot 0 owns (R, R-1).
// Every step each ring player advances one position, so an off-diagonal G
// entry at positions (P1, P2) moves to (P1+1, P2+1) (mod R; R stays R).
// Storing G by POSITION pair -- double-buffered, the update phase reads step
// st's buffer at the block's positions and writes the moved entries into the
// other buffer -- makes every thread's LDS addresses static for the whole
// kernel: no per-step index arithmetic.  Which entries of a block hold the
// next step's pairs is static as well (next_meeting).
template <int W>
struct Ord<W, EVD_CYCLIC> {
  static constexpr int R = 2 * W - 1;
  __host__ __device__ static constexpr int pos_next(int P) {
    return P == R ? P : (P + 1 == R ? 0 : P + 1);
  }
  __host__ __device__ static constexpr int prev_pos(int P) {
    return P == R ? P : (P == 0 ? R - 1 : P - 1);
  }
  __host__ __device__ static constexpr int slot_of(int pos) {  // slot of a position
    return pos == R ? 0 : (pos <= W - 2 ? pos + 1 : 2 * W - 2 - pos);
  }
  // Where the players now at positions (P1, P2) meet at the NEXT step: returns
  // 2*slot + (the player at P1 is that slot's first), or -1 if they do not.
  __host__ __device__ static constexpr int next_meeting(int P1, int P2) {
    if (P1 == R || P2 == R) {
      const int o = P1 == R ? P2 : P1;
      if (pos_next(o) != R - 1) return -1;  // N-1 meets the second of slot 0
      return P1 == R ? 1 : 0;
    }
    const int n1 = pos_next(P1), n2 = pos_next(P2);
    if (slot_of(n1) != slot_of(n2)) return -1;
    return 2 * slot_of(n1) + (n1 <= W - 2 ? 1 : 0);
  }
  // Position of player x at step 0 (inverse of players at st = 0).
  __host__ __device__ static constexpr int pos0(int x) { return x == R ? R : (x == 0 ? R - 1 : x - 1); }
  __host__ __device__ static constexpr int first_pos(int a) { return a == 0 ? R : a - 1; }
  __host__ __device__ static constexpr int second_pos(int a) { return 2 * W - 2 - a; }
  __host__ __device__ static constexpr int first0(int a) { return a == 0 ? R : a; }
  __host__ __device__ static constexpr int second0(int a) { return a == 0 ? 0 : R - a; }
  // Players of slot a at step st (the same movement as the DPP shifts of the
  // register Q: firsts move right, seconds left, player N-1 fixed in slot 0):
  // the player at ring position x after st steps is ((x - st) mod R + 1) mod R.
  // Checked against the DPP movement by
  // tests/test_schedule.py::test_evd_ring_matches_dpp_movement.
  __device__ static __forceinline__ int player(int pos, int st) {
    int x = pos - st;
    x += x < 0 ? R : 0;
    return x + 1 == R ? 0 : x + 1;
  }
  __device__ static void players(int a, int st, int& p, int& q) {
    p = a == 0 ? R : player(a - 1, st);
    q = player(second_pos(a), st);
  }
  // firsts shift right, seconds shift left; slot 0's first (player 2W-1)
  // stays, slot 1 takes slot 0's second, slot W-1's second is its own first
  template <typename V>
  __device__ static void move(V& f, V& s, int slot) {
    const V f_r = dpp_shr1(f), s_r = dpp_shr1(s), s_l = dpp_shl1(s);
    const V nf = slot == 0 ? f : (slot == 1 ? s_r : f_r);
    const V ns = slot == W - 1 ? f : s_l;
    f = nf;
    s = ns;
  }
};
// Lane i <- lane i+1 with wrap (DPP wave_rol:1).
__device__ __forceinline__ int dpp_rol1(int v) {
  return __builtin_amdgcn_mov_dpp(v, 0x134, 0xf, 0xf, false);
}
// Lane i <- lane i ^ 32 (v_permlane32_swap of a value with itself).
__device__ __forceinline__ int half_swap(int v) {
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return (threadIdx.x & 32) ? (int)r[0] : (int)r[1];
}
template <int W>
__device__ __forceinline__ int bip_shift(int v, int slot) {  // slot a <- slot a+1 (mod W)
  const int r = dpp_rol1(v);
  if constexpr (W == 32) return slot == W - 1 ? half_swap(r) : r;  // two slot groups per wave
  return r;
}
template <int W>
__device__ __forceinline__ float bip_shift(float v, int slot) {
  return __int_as_float(bip_shift<W>(__float_as_int(v), slot));
}
template <int W>
__device__ __forceinline__ double bip_shift(double v, int slot) {
  const long long x = __double_as_longlong(v);
  const int lo = bip_shift<W>((int)(x & 0xffffffff), slot), hi = bip_shift<W>((int)(x >> 32), slot);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int W>
struct Ord<W, EVD_BIP> {
  static_assert(W == 32 || W == 64 || W <= 16, "bipartite Q movement: one or two slot groups per wave");
  static constexpr int R = W;
  __host__ __device__ static constexpr int pos_next(int P) {
    return P < W ? P : (P == W ? 2 * W - 1 : P - 1);
  }
  __host__ __device__ static constexpr int prev_pos(int P) {
    return P < W ? P : (P == 2 * W - 1 ? W : P + 1);
  }
  __host__ __device__ static constexpr int slot_of(int pos) { return pos < W ? pos : pos - W; }
  __host__ __device__ static constexpr int next_meeting(int P1, int P2) {
    const int n1 = pos_next(P1), n2 = pos_next(P2);
    if ((n1 < W) == (n2 < W) || slot_of(n1) != slot_of(n2)) return -1;
    return 2 * slot_of(n1) + (n1 < W ? 1 : 0);
  }
  __host__ __device__ static constexpr int pos0(int x) { return x; }
  __host__ __device__ static constexpr int first_pos(int a) { return a; }
  __host__ __device__ static constexpr int second_pos(int a) { return W + a; }
  __host__ __device__ static constexpr int first0(int a) { return a; }
  __host__ __device__ static constexpr int second0(int a) { return W + a; }
  __device__ static void players(int a, int st, int& p, int& q) {
    p = a;
    q = W + (a + st) % W;
  }
  template <typename V>
  __device__ static void move(V& f, V& s, int slot) {
    (void)f;
    s = bip_shift<W>(s, slot);
  }
};
template <int W, int ORD>
__host__ __device__ constexpr int block_duty(int a, int b) {  // 256*e + meeting, or -1
  using O = Ord<W, ORD>;
  for (int e = 0; e < 4; ++e) {
    const int x = (e >> 1) ? O::second_pos(a) : O::first_pos(a);
    const int y = (e & 1) ? O::second_pos(b) : O::first_pos(b);
    const int mt = O::next_meeting(x, y);
    if (mt >= 0) return 256 * e + mt;
  }
  return -1;
}

// Which slot-pair blocks (a < b) each thread owns, computed at compile time.
// Thread roles: the W blocks holding the next step's pairs ("duty" blocks:
// their owners solve the rotations, W = 32 / 64 of them) go to the first W
// lanes of wave 0 -- the only lanes that solve, so only wave 0 carries the
// solve latency and it does no Q work; the other blocks follow in rows taken
// in complementary pairs 0, W-2, 1, W-3, ... (two paired rows hold W blocks,
// so a wave's lanes share few slots and the record reads broadcast).
// blk[j * NT + t] = (a << 8) | b of thread t's j-th block, 0xffff if none.
// OPT (fp32, bipartite, 1024 threads): the table of tools/evd_deal_opt.py
// instead -- the same duty blocks, the other blocks placed so the 32 lanes of
// each LDS lane group hit distinct banks where possible (modelled LDS cycles
// per step W=64: 1144 -> 812, conflict share 45 -> 22 %).
template <int W, int NT, int ORD = EVD_CYCLIC, bool OPT = false>
struct EvdDeal {
  static constexpr int NOFF = W * (W - 1) / 2;
  static constexpr int MAXOFF = (NOFF + NT - 1) / NT;
  unsigned short blk[MAXOFF * NT];
  constexpr EvdDeal() : blk{} {
    if constexpr (OPT) {
      static_assert(ORD == EVD_BIP && NT == 1024 && (W == 32 || W == 64), "optimised dealing tables");
      const unsigned short* t = W == 64 ? kEvdDealF32_W64_bip : kEvdDealF32_W32_bip;
      for (int g = 0; g < MAXOFF * NT; ++g) blk[g] = t[g];
      return;
    }
    using O = Ord<W, ORD>;
    int g = 0;
    // duty block of each next-step slot s: the positions that slot's players
    // occupy NOW are one behind its own positions
    for (int s = 0; s < W; ++s) {
      int a = O::slot_of(O::prev_pos(O::first_pos(s))), b = O::slot_of(O::prev_pos(O::second_pos(s)));
      if (a > b) {
        const int x = a;
        a = b;
        b = x;
      }
      blk[g++] = (unsigned short)((a << 8) | b);
    }
    for (int i = 0; i < W - 1; ++i) {
      const int a = (i & 1) ? W - 2 - (i >> 1) : (i >> 1);
      for (int b = a + 1; b < W; ++b)
        if (block_duty<W, ORD>(a, b) < 0) blk[g++] = (unsigned short)((a << 8) | b);
    }
    for (; g < MAXOFF * NT; ++g) blk[g] = 0xffff;
  }
};

// Compile-time check of the dealing: the first W entries are the duty blocks
// of next-step slots 0..W-1, and every block is dealt exactly once.
template <int W, int NT, int ORD, bool OPT = false>
constexpr bool evd_deal_ok() {
  constexpr EvdDeal<W, NT, ORD, OPT> d{};
  int seen[W * W] = {};
  int dealt = 0;
  for (int g = 0; g < EvdDeal<W, NT, ORD, OPT>::MAXOFF * NT; ++g) {
    if (d.blk[g] == 0xffff) continue;
    const int a = d.blk[g] >> 8, b = d.blk[g] & 255;
    if (!(a < b && b < W) || seen[a * W + b]++) return false;
    ++dealt;
    const int duty = block_duty<W, ORD>(a, b);
    if (g < W && (duty < 0 || ((duty & 255) >> 1) != g)) return false;
    if (g >= W && duty >= 0) return false;
  }
  return dealt == EvdDeal<W, NT, ORD, OPT>::NOFF;
}
static_assert(evd_deal_ok<32, kEvdThreads, EVD_CYCLIC>(), "EVD block dealing");
static_assert(evd_deal_ok<64, kEvdThreads, EVD_CYCLIC>(), "EVD block dealing");
static_assert(evd_deal_ok<32, kEvdThreads, EVD_BIP>(), "EVD block dealing");
static_assert(evd_deal_ok<64, kEvdThreads, EVD_BIP>(), "EVD block dealing");
static_assert(evd_deal_ok<64, 1024, EVD_BIP, true>(), "optimised EVD block dealing");
static_assert(evd_deal_ok<32, 1024, EVD_BIP, true>(), "optimised EVD block dealing");
// which dealing a kernel uses
template <typename T, int W, int NT, int ORD>
__host__ __device__ constexpr bool evd_deal_opt() {
  return sizeof(T) == 4 && ORD == EVD_BIP && NT == 1024 && (W == 32 || W == 64);
}

// ---- pre-pass and tail shared by evd_kernel and evd_cross_kernel.
// While a thread assembles G it folds every coupling g of columns with
// squared norms (g_rr, g_cc) into the step's convergence value
// max |g| / sqrt(g_rr g_cc) (columns under the floor left out, as in
// needs_rotation) and into "does any pair pass the rotation test".
template <typename T>
struct AssemblyFold {
  const T tol;
  const int absmode;
  const T nfloor;
  float mx = 0.0f;
  int need = 0;
  __device__ __forceinline__ void add(T g, T grr, T gcc) {
    const T d = sqrt(grr) * sqrt(gcc);
    if (d > T(0) && (absmode || (grr > nfloor && gcc > nfloor))) {
      const float v = (float)(fabs(g) / d);
      mx = v > mx ? v : mx;
    }
    need |= needs_rotation(grr, gcc, g, tol, absmode, nfloor) ? 1 : 0;
  }
  // Workgroup reduce (two barriers) through the kernel's LDS words, one per
  // wave: the convergence value into metric[0]; returns whether any thread's
  // entries need a rotation.
  template <int NWAVE>
  __device__ __forceinline__ bool reduce(float (&wmax)[NWAVE], int (&wneed)[NWAVE], int& need_any,
                                         uint32_t* metric) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    mx = wave_max(mx);
    need = __any(need) ? 1 : 0;
    if (lane == 0) {
      wmax[wave] = mx;
      wneed[wave] = need;
    }
    __syncthreads();
    if (tid == 0) {
      float m2 = 0.0f;
      int n2 = 0;
      for (int w = 0; w < NWAVE; ++w) {
        m2 = wmax[w] > m2 ? wmax[w] : m2;
        n2 |= wneed[w];
      }
      atomic_max_pos(&metric[0], m2);
      need_any = n2;
    }
    __syncthreads();
    return need_any != 0;
  }
};
// After the steps: the second-order stop test's inputs (svdj_stop.h) from the
// solver lanes of wave 0 -- largest effective sine into metric[4], rotation
// count into metric[5] -- the pair's skip flag and the count of pairs that
// rotated (metric[1]).  `any`: some inner sweep rotated.
__device__ __forceinline__ void evd_tail(bool any, float smax, uint32_t rcount, int pair,
                                         int32_t* skip, uint32_t* metric) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave == 0 && any) {
    const float sm = wave_max(smax);
    const uint32_t rc = wave_sum(rcount);
    if (lane == 0) {
      atomic_max_pos(&metric[4], sm);
      atomicAdd(&metric[5], rc);
    }
  }
  if (tid == 0) {
    skip[pair] = any ? 0 : 1;
    if (any) atomicAdd(&metric[1], 1u);
  }
}

template <typename T, int W, int ORD>
__global__ __launch_bounds__(kEvdThreads) void evd_kernel(
    const int32_t* __restrict__ pairs, int full, const T* __restrict__ slabs, int nchunk,
    T* __restrict__ D, T* __restrict__ Qout, int32_t* __restrict__ skip, T tol, int absmode,
    int max_inner, uint32_t* __restrict__ metric, int group_blocks = 0) {
  constexpr int NT = kEvdThreads;
  constexpr int NWAVE = NT / SVDJ_WAVE;
  constexpr int N = 2 * W;
  using O = Ord<W, ORD>;
  constexpr int R = O::R;               // steps per sweep
  constexpr int NTRI = N * (N - 1) / 2;
  constexpr int GPW = SVDJ_WAVE / W;    // Q row groups per wave
  // Q row groups: waves 1..NWAVE-1 (wave 0 solves).  Giving the solver wave
  // Q rows as well measured neutral (round 2, profiles/r2_evd_unroll): the
  // step is bound by the G update's LDS traffic, not by the Q rows.
  constexpr int QW0 = 1;  // first Q wave
  constexpr int NGRP = (NWAVE - QW0) * GPW;
  constexpr int RPL = (N + NGRP - 1) / NGRP;  // Q rows per lane (the last group may idle)
  constexpr bool DOPT = evd_deal_opt<T, W, NT, ORD>();
  constexpr int MAXOFF = EvdDeal<W, NT, ORD, DOPT>::MAXOFF;
  static_assert(W >= 4 && W <= 64 && NWAVE >= 2, "EVD geometry");
  using QT = double;  // fp32 Q measured 8 % faster with 10x worse V orthogonality
  static constexpr EvdDeal<W, NT, ORD, DOPT> deal{};

  __shared__ T Gb[2][NTRI + 1];  // off-diagonal G by position pair, double-buffered;
                                 // element NTRI takes the writes that go nowhere
  __shared__ T dg[N];        // assembled diagonal (player order)
  // rotation records by global step parity (structure of arrays): (c, s) in
  // the data precision steer G, (cq, sq) in the Q precision rotate Q (fp64
  // for fp32 data: normalised once, by the solver), (dp, dq) are the slot's
  // diagonals after its rotation
  // records as pairs: one 8/16-byte LDS access per (c, s), (dp, dq), (cq, sq)
  using T2 = Pair2<T>;
  using QT2 = Pair2<QT>;
  __shared__ T2 rcs[2][W], rdd[2][W];
  __shared__ QT2 rq[2][W];
  __shared__ int rot_flag[2];  // any rotation in sweep (parity), written by wave 0
  __shared__ float wmax[NWAVE];
  __shared__ int wneed[NWAVE];
  __shared__ int need_any;

  const int pair = blockIdx.x;
  const int bi = pairs[2 * pair], bj = pairs[2 * pair + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // grouped metrics (svdj_block_steps_grouped): the pair's matrix has its own words
  metric += group_blocks ? (bi / group_blocks) * SVDJ_METRIC_WORDS : 0;
  const T nfloor = norm_floor<T>(metric);

  // ---- assemble G: diagonal first (player order), then every off-diagonal
  // entry into position space for step 0; split-K slabs summed in fp64
  if (full) {
    const T* s0 = slabs + (size_t)pair * nchunk * (4 * W * W);
    for (int a = tid; a < N; a += NT) {
      double acc = 0;
      for (int c = 0; c < nchunk; ++c) acc += (double)s0[(size_t)c * 4 * W * W + a * N + a];
      dg[a] = (T)acc;
    }
  } else {
    for (int a = tid; a < N; a += NT) dg[a] = D[a < W ? bi * W + a : bj * W + (a - W)];
  }
  __syncthreads();
  // store an entry at its step-0 position; fold it into the convergence
  // value and the "anything to rotate" test
  AssemblyFold<T> fold{tol, absmode, nfloor};
  auto visit = [&](int r, int c, T g) {
    Gb[0][tri_idx<N>(O::pos0(r), O::pos0(c))] = g;
    fold.add(g, dg[r], dg[c]);
  };
  // Slab sums with 16-byte loads, all chunks of a group in flight at once
  // (one dependent global load per entry and chunk was ~12 us per kernel).
  constexpr int EV = 16 / (int)sizeof(T);
  if (full) {
    const T* s0 = slabs + (size_t)pair * nchunk * (4 * W * W);
    for (int gi = tid; gi < N * N / EV; gi += NT) {
      const auto acc = slab_sum<SVDJ_EVD_SLAB_UNROLL>(s0, gi * EV, 4 * W * W, nchunk);
#pragma unroll
      for (int u = 0; u < EV; ++u) {
        const int i = gi * EV + u, r = i / N, c = i % N;
        if (r < c) visit(r, c, (T)acc[u]);
      }
    }
  } else {
    // couplings inside a block are zero (blocks are kept internally orthogonal)
    for (int i = tid; i < N * N; i += NT) {
      const int r = i / N, c = i % N;
      if (r < c && (c < W || r >= W)) Gb[0][tri_idx<N>(O::pos0(r), O::pos0(c))] = T(0);
    }
    const T* s0 = slabs + (size_t)pair * nchunk * (W * W);
    for (int gi = tid; gi < W * W / EV; gi += NT) {
      const auto acc = slab_sum<SVDJ_EVD_SLAB_UNROLL>(s0, gi * EV, W * W, nchunk);
#pragma unroll
      for (int u = 0; u < EV; ++u) {
        const int i = gi * EV + u;
        visit(i / W, W + i % W, (T)acc[u]);
      }
    }
  }
  // If no pair passes the rotation test, the first pass would rotate nothing
  // (G never changes): it is skipped exactly.
  const bool run = fold.reduce(wmax, wneed, need_any, metric);

  // ---- this thread's blocks and their static addresses
  int ba[MAXOFF], bb[MAXOFF];
  int rd[MAXOFF][4], wr[MAXOFF][4];  // read / write BYTE offsets into a G buffer (NTRI: no write)
  int pw = (int)sizeof(T) * NTRI, sv = -1;  // solve duty (256*e + meeting; j = 0 only), pending byte offset
#pragma unroll
  for (int j = 0; j < MAXOFF; ++j) {
    const int code = deal.blk[j * NT + tid];
    ba[j] = bb[j] = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) rd[j][e] = wr[j][e] = 0;
    if (code != 0xffff) {
      const int a = code >> 8, b = code & 255;
      ba[j] = a;
      bb[j] = b;
      const int pa[2] = {O::first_pos(a), O::second_pos(a)};
      const int pb[2] = {O::first_pos(b), O::second_pos(b)};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = pa[e >> 1], y = pb[e & 1];
        rd[j][e] = (int)sizeof(T) * tri_idx<N>(x, y);
        wr[j][e] = (int)sizeof(T) * tri_idx<N>(O::pos_next(x), O::pos_next(y));
        if (j == 0 && tid < W) {
          const int mt = O::next_meeting(x, y);
          if (mt >= 0) {
            wr[j][e] = (int)sizeof(T) * NTRI;  // within-slot entry next step: written one phase later
            pw = (int)sizeof(T) * tri_idx<N>(O::pos_next(O::pos_next(x)), O::pos_next(O::pos_next(y)));
            sv = 256 * e + mt;
          }
        }
      }
    }
  }
  T pend = T(0);

  // ---- slot layout state of the register Q (waves 1..NWAVE-1)
  const bool qlane = wave >= QW0;
  const int slot = lane % W;
  const int grp = (wave - QW0) * GPW + lane / W;
  int pf = O::first0(slot);   // first player of this slot
  int ps = O::second0(slot);  // second player
  QT qf[RPL], qs[RPL];
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int k = grp * RPL + i;
    qf[i] = (k == pf) ? QT(1) : QT(0);
    qs[i] = (k == ps) ? QT(1) : QT(0);
  }

  // ---- prologue: step 0's rotations from the assembled G
  // second-order stop test (svdj_stop.h): largest effective sine and count
  // of the rotations this solver lane solved (the final look-ahead rotation
  // included: conservative)
  float smax = 0.0f;
  uint32_t rcount = 0;
  auto publish = [&](int b, int ns, T c, T sn, T t, T dfp, T dsp) {
    smax = fmaxf(smax, eff_sine(sn, dfp, dsp));
    rcount += sn != T(0) ? 1u : 0u;
    rcs[b][ns] = T2{c, sn};
    rdd[b][ns] = T2{dfp, dsp};
    if constexpr (sizeof(QT) == sizeof(T)) {
      rq[b][ns] = QT2{c, sn};
    } else {  // fp64 (c, s) of the fp32 t, normalised in fp64
      const double td = (double)t, c64 = rsqrt64(fma(td, td, 1.0));
      rq[b][ns] = QT2{c64, td * c64};
    }
  };
  // rotations seen by this solver lane in the current / next inner sweep
  // (OR-reduced over wave 0 once per sweep: no per-step flag store)
  int racc = 0, racc_next = 0;
  if (run && tid < W) {
    const int fa = O::first_pos(tid), sa = O::second_pos(tid);
    int p, q;
    O::players(tid, 0, p, q);
    const T gpp = dg[p], gqq = dg[q];
    const T gpq = Gb[0][tri_idx<N>(fa, sa)];
    T c, s, t;
    const bool rot = rotation_fast(gpp, gqq, gpq, tol, absmode, nfloor, c, s, t);
    racc = rot;
    // thread tid's duty block holds next-step slot tid (EvdDeal), so phase 0's
    // pending write moves this coupling to its step-1 position
    pend = rot ? T(0) : gpq;
    publish(0, tid, c, s, t, gpp - t * gpq, gqq + t * gpq);
  }
  __syncthreads();

  // One block's update J^T G J (entries moved to their next-step positions)
  // and, for a duty block, the next step's rotation of its slot.  Split in a
  // read half and a compute/write half so a thread issues the LDS reads of
  // ALL its blocks before any write: Gb[b] and Gb[nb] are disjoint but the
  // compiler cannot prove it, so a fused per-block read-compute-write
  // serialises the read latency of every block.
  // G entry at byte offset `off` of buffer b (b is a compile-time constant in
  // the unrolled step loop, so the buffer base folds into the ds offset)
  auto gat = [&](int b, int off) -> T& {
    return *reinterpret_cast<T*>(reinterpret_cast<char*>(&Gb[b][0]) + off);
  };
  struct BlkIn {
    T g00, g01, g10, g11, ca, sa, cb, sb, dx, dy;
  };
  auto load_block = [&](int j, int b, bool duty, BlkIn& k) {
    k.g00 = gat(b, rd[j][0]);
    k.g01 = gat(b, rd[j][1]);
    k.g10 = gat(b, rd[j][2]);
    k.g11 = gat(b, rd[j][3]);
    const T2 ra = rcs[b][ba[j]], rb = rcs[b][bb[j]];
    k.ca = ra.x;
    k.sa = ra.y;
    k.cb = rb.x;
    k.sb = rb.y;
    k.dx = k.dy = T(0);
    if (duty) {
      const int e = sv >> 8;
      const T2 da = rdd[b][ba[j]], db = rdd[b][bb[j]];
      k.dx = (e >> 1) ? da.y : da.x;
      k.dy = (e & 1) ? db.y : db.x;
    }
  };
  auto finish_block = [&](int j, int nb, bool duty, bool last, const BlkIn& k) {
    const T h00 = k.ca * k.g00 - k.sa * k.g10, h01 = k.ca * k.g01 - k.sa * k.g11;
    const T h10 = k.sa * k.g00 + k.ca * k.g10, h11 = k.sa * k.g01 + k.ca * k.g11;
    const T h[4] = {k.cb * h00 - k.sb * h01, k.sb * h00 + k.cb * h01, k.cb * h10 - k.sb * h11,
                    k.sb * h10 + k.cb * h11};
    if (duty) {
      const int e = sv >> 8;
      const int ns = (sv & 255) >> 1;
      const bool x_first = sv & 1;
      const T g = e == 0 ? h[0] : e == 1 ? h[1] : e == 2 ? h[2] : h[3];
      const T df = x_first ? k.dx : k.dy, ds = x_first ? k.dy : k.dx;
      T c, sn, t;
      const bool rot = rotation_fast(df, ds, g, tol, absmode, nfloor, c, sn, t);
      if (last) racc_next |= rot; else racc |= rot;
      pend = rot ? T(0) : g;
      publish(nb, ns, c, sn, t, df - t * g, ds + t * g);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) gat(nb, wr[j][q]) = h[q];
  };
  auto update_blocks = [&](int b, int nb, bool solver, bool last) {
    BlkIn k[MAXOFF];
#pragma unroll
    for (int j = 0; j < MAXOFF; ++j)
      if (ba[j] >= 0) load_block(j, b, solver && j == 0 && sv >= 0, k[j]);
    // the coupling of this step's pair, solved last phase (or in the
    // prologue), moved on to its next-step position (dummy if no duty)
    gat(nb, pw) = pend;
#pragma unroll
    for (int j = 0; j < MAXOFF; ++j)
      if (ba[j] >= 0) finish_block(j, nb, solver && j == 0 && sv >= 0, last, k[j]);
  };

  bool any = false;
  int gs = 0;  // global step counter: step gs reads buffer gs & 1, records gs & 1
  int sw = 0, st = 0;
  // One step with the buffer parity as a compile-time constant (the loop
  // below alternates the two instantiations): every G / record address is a
  // loop-invariant register plus an immediate.  Returns true when done.
  auto step = [&](auto parity) -> bool {
    constexpr int b = decltype(parity)::value, nb = b ^ 1;
    const bool last = st + 1 == R;  // this phase solves step 0 of the next sweep
    if (wave == 0) {
      // solver wave: its duty blocks (lanes < W, j = 0) and nothing else of Q
      update_blocks(b, nb, true, last);
      if (last) {  // every rotation of sweep sw is decided by now
        const int rot = __any(racc) ? 1 : 0;
        if (lane == 0) rot_flag[sw & 1] = rot;
        racc = racc_next;
        racc_next = 0;
      }
    } else {
      // Q waves: this step's Q rotation (records read up front)
      const QT2 rqs = rq[b][slot];
      const QT cq = rqs.x, sq = rqs.y;
      update_blocks(b, nb, false, last);
      // Q <- Q J in registers (c = 1, s = 0 for no rotation)
#pragma unroll
      for (int i = 0; i < RPL; ++i) {
        const QT x = qf[i], y = qs[i];
        qf[i] = cq * x - sq * y;
        qs[i] = sq * x + cq * y;
      }
      // advance the ordering (DPP lane moves of the slot layout)
#pragma unroll
      for (int i = 0; i < RPL; ++i) O::move(qf[i], qs[i], slot);
      O::move(pf, ps, slot);
    }
    __syncthreads();
    ++gs;
    if (++st < R) return false;
    st = 0;
    if (!rot_flag[sw & 1]) return true;
    any = true;
    return ++sw >= max_inner;
  };
  if (run && max_inner > 0)
    while (!step(std::integral_constant<int, 0>{}) && !step(std::integral_constant<int, 1>{})) {
    }

  evd_tail(any, smax, rcount, pair, skip, metric);
  // Full mode re-measured the diagonal from the data: always refresh D.
  if (!any && !full) return;
  if (any) {
    if (qlane) {
      T* qo = Qout + (size_t)pair * N * N;
#pragma unroll
      for (int i = 0; i < RPL; ++i) {
        const int k = grp * RPL + i;
        if (k < N) {
          qo[k * N + pf] = (T)qf[i];
          qo[k * N + ps] = (T)qs[i];
        }
      }
    }
    // diagonals after the last executed step (records of step gs - 1)
    if (tid < W) {
      const int lb = (gs - 1) & 1;
      int p, q;
      O::players(tid, R - 1, p, q);
      D[p < W ? bi * W + p : bj * W + (p - W)] = rdd[lb][tid].x;
      D[q < W ? bi * W + q : bj * W + (q - W)] = rdd[lb][tid].y;
    }
  } else {
    for (int a = tid; a < N; a += NT) D[a < W ? bi * W + a : bj * W + (a - W)] = dg[a];
  }
}

// ----------------------------------------- evd, cross-only bipartite (mode 3)
// The EVD of a cross step that tracks only what the bipartite ordering
// reads: the W x W cross couplings C and the 2W diagonals.  When a cross
// step starts, each block's own columns are mutually orthogonal (the
// full-Gram step that opens every sweep rotates the within-block pairs), so
// G = [[Dx, C], [C^T, Dy]].  A rotation of (x_i, y) creates within-block
// couplings only at first order in its sine, and those feed back into the
// cross couplings at second order: the update
//   C'[i][j] = c_i c_k C[i][j] - s_i s_k C[k][pi(i)]     (y_j paired with x_k)
// drops them.  Near convergence the sines are tiny and the rotations are the
// exact ones; early on they differ slightly, which the next outer visit of
// the pair re-measures from the data.  CPU emulation (fp32 / fp64, n = 512 /
// 1024, W = 32 / 64): the same sweep counts as the full bipartite EVD +-1,
// the same accuracy.
//
// Position space: at step t, Y position p holds y_{(p + t) mod W}; slot a
// pairs x_a with position a.  E[i][p] = C[i][y at p].  The update pairs
// E[i][p] with E[p][i] (a STATIC transpose pair) and the new values move
// one position left: E_{t+1}[i][p] = E'_t[i][p+1].  Groups {E[i][i+d],
// E[i+d][i]} along diagonals d = 1..W/2:
//   * wave 0, lane a = slot a, holds d = 1 and d = 2 in REGISTERS: its next
//     active coupling E_{t+1}[a][a] = E'_t[a][a+1] needs only values of
//     lanes a+1 and a+2 (their rotations, E_t[a+1][a] = lane a+1's settled
//     coupling, E_t[a+2][a] = lane a+1's previous d = 1 result), fetched
//     with DPP lane rotates -- the solve chain has no LDS read on it;
//   * waves 1.. hold d = 3..W/2 in LDS (row stride W, bank-conflict-free),
//     two diagonals per wave; the d = 2 / d = 3 values cross through LDS.
// ONE barrier per step.  The kernel does not accumulate Q: every step's
// rotations go to global memory as tangent records, and qbuild_kernel forms
// the fp64 (c, s) and Q = J_0 J_1 ... row-parallel on many CUs (rows of Q
// evolve independently).  Measured in isolation (tools/micro/evd_bench.hip, 8
// pairs, W = 64): register Q accumulation and the solve chain made the
// per-step time ~2000 cycles; the G update itself was not the limit.  Round
// 6 ablations (profiles/r6_evd): of 33 us per launch, 14 us are barriers,
// lane rotates, bookkeeping, assembly and launch; the records cost 3.8 us
// (their fp64 (c, s), now formed by the Q builds, and the per-step wait for
// their stores), the rotation solve 6 us.
// DPW: coupling diagonals per wave >= 1 (W = 64; W = 32 keeps 2, one per lane half)
template <int W, int DPW = 2>
__host__ __device__ constexpr int cross_threads() {
  return W == 64 ? SVDJ_WAVE * (1 + (W / 2 - 2 + DPW - 1) / DPW) : 512;
}

// ABL (tools/micro/evd_bench.hip only; production launches ABL = 0): bit 0
// no rotation records; bit 1 waves >= 1 skip their coupling updates
// (barriers kept); bit 2 the solver lane skips the rotation (c = 1, s = 0);
// bit 3 the solver lane skips its LDS coupling read and write; bit 4 no
// steps at all (assembly, launch and the epilogue only).
template <typename T, int W, int ABL = 0, int DPW = 2>
__global__ __launch_bounds__((cross_threads<W, DPW>())) void evd_cross_kernel(
    const int32_t* __restrict__ pairs, const T* __restrict__ slabs, int nchunk,
    T* __restrict__ D, T* __restrict__ rec, int32_t* __restrict__ nsteps,
    int32_t* __restrict__ skip, T tol, int absmode, int max_inner, uint32_t* __restrict__ metric,
    int group_blocks = 0) {
  static_assert(W == 32 || W == 64, "cross EVD: W = 32 or 64");
  static_assert(W == 64 || DPW == 2, "W = 32: two diagonals per wave (one per lane half)");
  constexpr int NT = cross_threads<W, DPW>();
  constexpr int NWAVE = NT / SVDJ_WAVE;
  static_assert(W == 32 ? NWAVE - 1 == (W / 2 - 2) / 2 : NWAVE - 1 == (W / 2 - 2 + DPW - 1) / DPW,
                "DPW diagonals per wave >= 1");
  constexpr int N = 2 * W;
  using T2 = Pair2<T>;

  __shared__ T Eb[2][W * W];  // cross couplings by (x slot, y position), double-buffered
  __shared__ T dg[N];
  __shared__ T2 rcs[2][W];
  __shared__ int rot_flag[2];
  __shared__ float wmax[NWAVE];
  __shared__ int wneed[NWAVE];
  __shared__ int need_any;

  const int pair = blockIdx.x;
  const int bi = pairs[2 * pair], bj = pairs[2 * pair + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // grouped metrics (svdj_block_steps_grouped): the pair's matrix has its own words
  metric += group_blocks ? (bi / group_blocks) * SVDJ_METRIC_WORDS : 0;
  const T nfloor = norm_floor<T>(metric);

  // ---- assemble: diagonals from D, E_0[i][p] = C[i][p] (split-K slabs
  // summed in fp64), convergence value and the "anything to rotate" test
  for (int a = tid; a < N; a += NT) dg[a] = D[a < W ? bi * W + a : bj * W + (a - W)];
  __syncthreads();
  AssemblyFold<T> fold{tol, absmode, nfloor};
  constexpr int EV = 16 / (int)sizeof(T);
  const T* s0 = slabs + (size_t)pair * nchunk * (W * W);
  for (int gi = tid; gi < W * W / EV; gi += NT) {
    const auto acc = slab_sum<SVDJ_EVD_SLAB_UNROLL>(s0, gi * EV, W * W, nchunk);
#pragma unroll
    for (int u = 0; u < EV; ++u) {
      const int i = gi * EV + u;
      const T g = (T)acc[u];
      Eb[0][i] = g;
      fold.add(g, dg[i / W], dg[W + i % W]);
    }
  }
  const bool run = fold.reduce(wmax, wneed, need_any, metric) && (ABL & 16) == 0;
  const int inner = max_inner < kCrossMaxInner ? max_inner : kCrossMaxInner;

  // ---- LDS groups of waves >= 1: (i, d), d = DPW (w - 1) + 3 + j (W = 64:
  // all on every lane; W = 32: d = 2w+1 on lanes 0..31, 2w+2 on 32..63);
  // gv bit j: group j exists on this lane (the half diagonal has W/2 groups)
  constexpr int G = W == 64 ? DPW : 1;
  int gi[G], gp[G], rd0[G], rd1[G], wr0[G], wr1[G];
  uint32_t gv = 0;
#pragma unroll
  for (int jg = 0; jg < G; ++jg) {
    const int i = W == 64 ? lane : (lane & 31);
    const int d = W == 64 ? DPW * (wave - 1) + 3 + jg : 2 * wave + 1 + (lane >> 5);
    const bool ok = wave >= 1 && d <= W / 2 && !(d == W / 2 && i >= W / 2);
    const int p = (i + d) % W;
    gi[jg] = i;
    gp[jg] = p;
    rd0[jg] = i * W + p;
    rd1[jg] = p * W + i;
    wr0[jg] = i * W + (p + W - 1) % W;
    wr1[jg] = p * W + (i + W - 1) % W;
    gv |= ok ? 1u << jg : 0u;
  }

  // ---- solver lanes (wave 0, lane a < W): slot a's state in registers
  const bool solver = wave == 0 && lane < W;
  const int a = lane % W;
  T rc = T(1), rs = T(0);   // rotation of slot a at the current step
  T rdx = T(0), rdy = T(0); // x_a / y at position a after the current step's rotation
  T pend = T(0);            // slot a's coupling after the current step's rotation
  T pend_prev = T(0);       // ... after the previous step: E_t[a][a-1]
  T g1 = T(0);              // E_t[a][a+1]
  T h2src = T(0);           // E_t[a+1][a-1] (lane a-1's E_t[(a-1)+2][a-1])
  T dx_out = T(0), dy_out = T(0);
  T* rq = rec + (size_t)pair * (kCrossMaxInner * W) * W;
  T rt = T(0);  // tangent of the latest solved rotation; its fp64 record is
                // written at the start of the next phase (steps 0 .. gs-1 are
                // recorded; the look-ahead rotation solved in the final phase
                // is never used)
  // second-order stop test (svdj_stop.h): largest effective sine and count
  // of the rotations applied (recorded); the effective sine of the latest
  // solved rotation is formed when it is recorded, off the solve chain
  float smax = 0.0f;
  uint32_t rcount = 0;
  auto solve = [&](T dx, T dy, T g, bool& rot) {
    T c, sn, t;
    if constexpr ((ABL & 4) != 0) {
      rot = false;
      c = T(1);
      sn = t = T(0);
    } else {
      rot = rotation_fast(dx, dy, g, tol, absmode, nfloor, c, sn, t);
    }
    rc = c;
    rs = sn;
    rt = t;
    rdx = dx - t * g;
    rdy = dy + t * g;
    pend = rot ? T(0) : g;
  };
  auto record = [&](int step) {  // before the next solve: rs, rdx, rdy still its inputs'
    smax = fmaxf(smax, eff_sine(rs, rdx, rdy));
    rcount += rs != T(0) ? 1u : 0u;
    if constexpr ((ABL & 1) != 0) return;
    // the tangent only: the Q builds form the fp64 (c, s) from it
    // (rotation_cs), off this lane's step
    if (step < kCrossMaxInner * W) rq[(size_t)step * W + a] = rt;
  };
  int racc = 0, racc_next = 0;
  if (run && solver) {  // step 0 of slot a
    pend_prev = Eb[0][a * W + (a + W - 1) % W];
    h2src = Eb[0][((a + 1) % W) * W + (a + W - 1) % W];
    g1 = Eb[0][a * W + (a + 1) % W];
    bool rot;
    solve(dg[a], dg[W + a], Eb[0][a * W + a], rot);
    racc = rot;
    rcs[0][a] = T2{rc, rs};
  }
  __syncthreads();

  bool any = false;
  int gs = 0, sw = 0, st = 0;
  auto step = [&](auto parity) -> bool {
    constexpr int b = decltype(parity)::value, nb = b ^ 1;
    const bool last = st + 1 == W;  // this phase solves step 0 of the next inner sweep
    if (wave == 0) {
      // neighbours' values (slot a+1, a+2) by lane rotates; E_t[a][a+2] from LDS
      const T g2 = solver && (ABL & 8) == 0 ? Eb[b][a * W + (a + 2) % W] : T(0);
      // fp64 record of step gs (solved in the previous phase) while the LDS
      // read is in flight: off the barrier-to-barrier critical path
      if (solver) record(gs);
      const T c1 = bip_shift<W>(rc, a), s1 = bip_shift<W>(rs, a);
      const T c2 = bip_shift<W>(c1, a), s2 = bip_shift<W>(s1, a);
      const T h1 = bip_shift<W>(pend_prev, a);  // E_t[a+1][a]
      const T h2 = bip_shift<W>(h2src, a);      // E_t[a+2][a]
      const T dyn = bip_shift<W>(rdy, a);       // y at position a+1 after this step
      if (solver) {
        const T cc1 = rc * c1, ss1 = rs * s1, cc2 = rc * c2, ss2 = rs * s2;
        const T n0_1 = cc1 * g1 - ss1 * h1;  // E_{t+1}[a][a]: slot a's next coupling
        const T n1_1 = cc1 * h1 - ss1 * g1;  // E_{t+1}[a+1][a-1]
        const T n0_2 = cc2 * g2 - ss2 * h2;  // E_{t+1}[a][a+1]
        const T n1_2 = cc2 * h2 - ss2 * g2;  // E_{t+1}[a+2][a-1] (a d = 3 group's input)
        if constexpr ((ABL & 8) == 0) Eb[nb][((a + 2) % W) * W + (a + W - 1) % W] = n1_2;
        dx_out = rdx;
        dy_out = rdy;
        pend_prev = pend;
        g1 = n0_2;
        h2src = n1_1;
        bool rot;
        solve(rdx, dyn, n0_1, rot);
        if (last) racc_next |= rot; else racc |= rot;
        rcs[nb][a] = T2{rc, rs};
      }
      if (last) {  // every rotation of inner sweep sw is decided by now
        const int r = __any(racc) ? 1 : 0;
        if (lane == 0) rot_flag[sw & 1] = r;
        racc = racc_next;
        racc_next = 0;
      }
    } else if constexpr ((ABL & 2) == 0) {
      T e0[G], e1[G];
      T2 ri[G], rp[G];
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (gv >> j & 1u) {
          e0[j] = Eb[b][rd0[j]];
          e1[j] = Eb[b][rd1[j]];
          ri[j] = rcs[b][gi[j]];
          rp[j] = rcs[b][gp[j]];
        }
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (gv >> j & 1u) {
          const T cc = ri[j].x * rp[j].x, ss = ri[j].y * rp[j].y;
          Eb[nb][wr0[j]] = cc * e0[j] - ss * e1[j];
          Eb[nb][wr1[j]] = cc * e1[j] - ss * e0[j];
        }
    }
    // LDS-only barrier: __syncthreads would also wait for the record stores
    // (vmcnt(0)) every step; nothing in the loop reads global memory
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    ++gs;
    if (++st < W) return false;
    st = 0;
    if (!rot_flag[sw & 1]) return true;
    any = true;
    return ++sw >= inner;
  };
  if (run && inner > 0)
    while (!step(std::integral_constant<int, 0>{}) && !step(std::integral_constant<int, 1>{})) {
    }

  evd_tail(any, smax, rcount, pair, skip, metric);
  if (tid == 0) nsteps[pair] = gs;
  if (any && solver) {  // diagonals after the last executed step (gs - 1)
    D[bi * W + a] = dx_out;
    D[bj * W + ((a + gs - 1) & (W - 1))] = dy_out;
  }
}

// Q = J_0 J_1 ... J_{steps-1} of a cross-step EVD from its fp64 rotation
// records (evd_cross_kernel), row-parallel: row k of Q evolves on its own
// (q_k <- q_k J_t), so a pair's 2W rows spread over several workgroups and
// CUs instead of sitting in the EVD workgroup's registers.  Lane = slot a
// (W = 32: two slot groups per wave); per row and step one 2x2 fp64 rotation
// of (Q[k][x_a], Q[k][y at position a]) and a lane rotate of the y column
// (position a takes what position a+1 held).  The records of up to 64 steps
// are staged in LDS first with wide loads (one global latency instead of
// one per step: read step by step from L2 the kernel was latency bound),
// then read two steps ahead.  Rounded to the data type once, at the end.
// R rows per lane: 4 when a step has few pairs (latency: more workgroups per
// pair), 16 with many pairs (throughput: each workgroup stages the pair's
// records once for 4x the rows).
constexpr int kQbThreads = 256;
constexpr int kQbChunk = 64;  // steps staged in LDS at a time
// fp64 (c, s) of a recorded tangent (evd_cross_kernel records t only):
// fp32 data -- the fp32 t normalised in fp64 (Q stays orthogonal to fp64
// rounding); fp64 data -- rotation_fast's own c = 1 / sqrt(1 + t^2), s = t c.
__device__ __forceinline__ Pair2<double> rotation_cs(float t) {
  const double td = (double)t, c = rsqrt64(fma(td, td, 1.0));
  return Pair2<double>{c, td * c};
}
__device__ __forceinline__ Pair2<double> rotation_cs(double t) {
  const double c = 1.0 / sqrt(fma(t, t, 1.0));
  return Pair2<double>{c, t * c};
}
// The rotation loop of the Q builds (qbuild_kernel, qbuild_quad_kernel): the
// ns recorded steps of one pair (tangents at rp, W per step) applied to this
// lane's R rows of the columns of slot a -- qx[i] the x column, qy[i] the y
// column at position a.  NT threads stage kQbChunk steps at a time in rs as
// fp64 (c, s); every thread of the workgroup calls it (barriers).
template <int W, int R, int NT, typename T>
__device__ __forceinline__ void qbuild_rotate(const T* rp, int ns, Pair2<double> (&rs)[kQbChunk * W],
                                              int a, double (&qx)[R], double (&qy)[R]) {
  using Q2 = Pair2<double>;
  // One chunk as a lambda: written straight into the chunk loop, the compiler
  // waited for the look-ahead read of step t + 2 right after issuing it in
  // most instantiations (profiles/evd_shared, read from the assembly).
  auto chunk = [&](int t0) {
    const int nc = ns - t0 < kQbChunk ? ns - t0 : kQbChunk;
    for (int i = threadIdx.x; i < nc * W; i += NT) rs[i] = rotation_cs(rp[(size_t)t0 * W + i]);
    __syncthreads();
    Q2 n0 = rs[a], n1 = nc > 1 ? rs[W + a] : Q2{1.0, 0.0};
    for (int t = 0; t < nc; ++t) {
      const Q2 cs = n0;
      n0 = n1;
      if (t + 2 < nc) n1 = rs[(t + 2) * W + a];
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const double x = qx[i], y = qy[i];
        qx[i] = cs.x * x - cs.y * y;
        qy[i] = bip_shift<W>(cs.y * x + cs.x * y, a);
      }
    }
    __syncthreads();  // the next chunk overwrites rs
  };
  for (int t0 = 0; t0 < ns; t0 += kQbChunk) chunk(t0);
}
template <int W, int R>
__host__ __device__ constexpr int qbuild_blocks() {  // workgroups per pair
  return (2 * W) / (R * (SVDJ_WAVE / W) * (kQbThreads / SVDJ_WAVE));
}
template <typename T, int W, int R>
__global__ __launch_bounds__(kQbThreads) void qbuild_kernel(
    const T* __restrict__ rec, const int32_t* __restrict__ nsteps,
    const int32_t* __restrict__ skip, T* __restrict__ Qall) {
  constexpr int N = 2 * W;
  constexpr int GPW = SVDJ_WAVE / W;
  static_assert(qbuild_blocks<W, R>() * R * GPW * (kQbThreads / SVDJ_WAVE) == N, "row cover");
  using Q2 = Pair2<double>;
  __shared__ Q2 rs[kQbChunk * W];
  const int pair = blockIdx.x;
  if (skip[pair]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = lane % W;
  const int k0 = ((blockIdx.y * (kQbThreads / SVDJ_WAVE) + wave) * GPW + lane / W) * R;
  const int ns = nsteps[pair];
  const T* rp = rec + (size_t)pair * (kCrossMaxInner * W) * W;
  double qx[R], qy[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    qx[i] = (k0 + i == a) ? 1.0 : 0.0;
    qy[i] = (k0 + i == W + a) ? 1.0 : 0.0;
  }
  qbuild_rotate<W, R, kQbThreads>(rp, ns, rs, a, qx, qy);
  T* qo = Qall + (size_t)pair * N * N;
  const int yc = W + (a + ns) % W;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    qo[(k0 + i) * N + a] = (T)qx[i];
    qo[(k0 + i) * N + yc] = (T)qy[i];
  }
}

}  // namespace svdj
