// Quad step of the block Jacobi sweep (block.hip): two consecutive cross
// steps fused (fp32, W = 64, split-bf16 apply) -- the Q builds, the Gram-space
// update, the T-stationary apply and the six-Gram kernel.
// The stage comment is at "quad step" below.
#pragma once
#include "block_apply.hpp"
#include "block_evd.hpp"
#include "block_gram.hpp"
#include "common.hpp"

namespace svdj {

// ------------------------------------------------------------- quad step
// Two consecutive cross steps fused (fp32, W = 64, split-bf16 apply).  Four
// W-blocks (a, b, c, d) = the block pairs (a,c),(b,d) of step s and
// (a,d),(b,c) of step s+1 (a super-block pair {a,b} x {c,d}, the schedule
// of parallel/schedule.py quad_round_robin / quad_bipartite).  Step s+1's
// couplings are formed in Gram space instead of from the data:
//   gram   : the six cross Grams C_ac, C_bd, C_ad, C_bc, C_ab, C_cd in ONE
//            launch (gram_quad_kernel: each block of the quad read once,
//            products instead of once per step);
//   evd 1  : evd_cross_kernel on (a,c), (b,d)  -> rotation records;
//   T1     : qbuild_quad_kernel<1> -> Q_ac, Q_bd in fp64;
//   update : C(a',d') = [Q_aa;Q_ca]^T [[C_ab,C_ad],[C_cb,C_cd]] [Q_bd;Q_dd] and
//            C(b',c') likewise (quad_update_kernel): exact in Gram space, the
//            within-pair blocks C_ab, C_cd included;
//   evd 2  : evd_cross_kernel on (a,d), (b,c) from those couplings;
//   T      : qbuild_quad_kernel<2> applies the step-(s+1) rotations to the
//            rows of T1 in fp64: T = T1 T2, the whole 256 x 256 transform;
//   apply  : [a b c d] <- [a b c d] T once, for A and V (apply_quad_ts_kernel).
// The data moves through HBM once per two steps instead of twice, and the
// apply contracts over K = 256 instead of 128: its split-bf16 MFMAs, no
// longer waiting on HBM, set the pace.  Numerically it is the two W-block
// steps with the same pairs (same EVDs, the couplings of step s+1 computed
// from the exact rotations of step s), and T is accumulated in fp64 and
// rounded once instead of twice.

// Q of an EVD pair (phase 1, rows of the pair, output fp64 T1) or the quad's
// T (phase 2: rows of all 4 blocks, starting from the phase-1 transforms,
// output T - I split into NP bf16 parts).  Same row-parallel rotation loop as
// qbuild_kernel; a skipped pair contributes the identity (phase 1 writes it:
// T1 is read by update and phase 2 even when its pair did not rotate).
// First element of the split T - I fragment (quad q, 32-row k block kb, 32-column
// tile ct, 16-column sub-tile cs) in the apply's A-operand layout
// (apply_quad_ts_kernel): NP parts of SVDJ_WAVE bf16x8 each; element e of lane
// 16g + i = (T - I)[32 kb + 8g + e][32 ct + 16 cs + i].
__host__ __device__ constexpr size_t ts_frag(int q, int kb, int ct, int cs, int np) {
  return ((((size_t)q * 8 + kb) * 8 + ct) * 2 + cs) * np * SVDJ_WAVE;
}

// Phase 2 writes T - I straight in the apply's split-bf16 fragment layout
// (round 6; a separate split pass over an fp32 T before): a thread's R rows
// k0 .. k0 + R - 1 of one column are elements k0 % 8 .. of one A-operand
// fragment (k block k0 / 32, lane group (k0 / 8) & 3).
template <int PHASE, int R, int NT, int NP = 0>
__global__ __launch_bounds__(NT) void qbuild_quad_kernel(
    const float* __restrict__ rec, const int32_t* __restrict__ nsteps,
    const int32_t* __restrict__ skip, double* __restrict__ T1, bf16x8* __restrict__ Ts = nullptr) {
  static_assert(PHASE == 1 ? NP == 0 : ((NP == 2 || NP == 3) && (R == 2 || R == 4 || R == 8)),
                "phase 2: split T - I, 2 / 4 / 8 rows per thread");
  constexpr int W = 64, N = 2 * W, QN = 4 * W;
  constexpr int WAVES = NT / SVDJ_WAVE;
  static_assert((PHASE == 1 ? N : QN) % (R * WAVES) == 0, "row cover");
  using Q2 = Pair2<double>;
  __shared__ Q2 rs[kQbChunk * W];
  const int pair = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = lane;
  const int k0 = (blockIdx.y * WAVES + wave) * R;
  const int ns = skip[pair] ? 0 : nsteps[pair];
  const float* rp = rec + (size_t)pair * (kCrossMaxInner * W) * W;
  const int q = pair >> 1, j = pair & 1;
  double qx[R], qy[R];
  if constexpr (PHASE == 1) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      qx[i] = (k0 + i == a) ? 1.0 : 0.0;
      qy[i] = (k0 + i == W + a) ? 1.0 : 0.0;
    }
  } else {
    // sub-pair j = 0: (a', d'), x = a' (column a of Q_ac), y = d' (column
    // W + a of Q_bd); j = 1: (b', c'), x = b' (Q_bd), y = c' (Q_ac).  Quad
    // row k is block k >> 6 in [a b c d] order: Q_ac holds rows of a, c (even
    // blocks), Q_bd rows of b, d (odd blocks).
    const double* tx = T1 + (size_t)(2 * q + j) * N * N;
    const double* ty = T1 + (size_t)(2 * q + 1 - j) * N * N;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int k = k0 + i, rb = k >> 6, kl = ((rb >> 1) << 6) + (k & 63);
      qx[i] = (rb & 1) == j ? tx[(size_t)kl * N + a] : 0.0;
      qy[i] = (rb & 1) != j ? ty[(size_t)kl * N + W + a] : 0.0;
    }
  }
  qbuild_rotate<W, R, NT>(rp, ns, rs, a, qx, qy);
  const int yr = (a + ns) & (W - 1);
  if constexpr (PHASE == 1) {
    double* qo = T1 + (size_t)pair * N * N;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      qo[(size_t)(k0 + i) * N + a] = qx[i];
      qo[(size_t)(k0 + i) * N + W + yr] = qy[i];
    }
  } else {  // element e of lane 16g + i of fragment (kb, ct, cs) = (T - I)[32 kb +
            // 8g + e][32 ct + 16 cs + i]; R < 8 rows per thread fill elements
            // k0 % 8 .. + R - 1 of the fragment
    using bfR = __attribute__((ext_vector_type(R))) __bf16;
    const int xc = (j == 0 ? 0 : W) + a, yc = (j == 0 ? 3 * W : 2 * W) + yr;
    const int kb = k0 >> 5, gg = (k0 >> 3) & 3, e0 = k0 & 7;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int col = side ? yc : xc;
      bfR parts[NP];
#pragma unroll
      for (int e = 0; e < R; ++e) {
        __bf16 pp[NP];
        // T rounded to fp32 first, then T - I (exact: |T| <= 1)
        const float t = (float)(side ? qy[e] : qx[e]) - (k0 + e == col ? 1.0f : 0.0f);
        split_bf16<NP>(t, pp);
#pragma unroll
        for (int pi = 0; pi < NP; ++pi) parts[pi][e] = pp[pi];
      }
      __bf16* dst = reinterpret_cast<__bf16*>(Ts + ts_frag(q, kb, col >> 5, (col >> 4) & 1, NP) +
                                              (col & 15) + 16 * gg) + e0;
#pragma unroll
      for (int pi = 0; pi < NP; ++pi) *reinterpret_cast<bfR*>(dst + pi * SVDJ_WAVE * 8) = parts[pi];
    }
  }
}

// Step-(s+1) couplings of quad q in Gram space, one workgroup per output
// pair and column half (blockIdx.x = 2q + j, blockIdx.y = oj): j = 0
// C(a',d') = L^T M R with L = Q_ac[:, :W] (rows a;c), M = [[C_ab, C_ad],
// [C_cb, C_cd]] (rows a;c, columns b;d), R = Q_bd[:, W:]; j = 1 C(b',c') =
// Q_bd[:, :W]^T M^T Q_ac[:, W:].  M is summed over the Gram's row chunks in
// fp64, R's and L's columns are staged in LDS (fp32), both products on f32
// MFMA (the data Gram is f32 MFMA as well).  Output: one W x W slab per pair
// of step s+1 (nchunk = 1), the layout evd_cross_kernel reads.
// NT = 512: the same MFMA waves (4, then 2), twice the loads in flight in the
// fill phases (the kernel is load-latency bound: 1 workgroup per CU).
template <int NT>
__global__ __launch_bounds__(NT) void quad_update_kernel(
    const float* __restrict__ slabs, int gch, const double* __restrict__ T1,
    float* __restrict__ upd) {
  constexpr int kUpdThreads = NT;
  // M's row stride is odd (129 = 1 mod 64 banks): its transposed fill and
  // both read orders are conflict-free (MP = N + 4 had 52 % bank-conflict
  // cycles, profiles/r5_prof_final)
  constexpr int W = 64, N = 2 * W, MP = N + 1, HP = 32 + 4;
  using M = Mfma<float>;
  __shared__ float Ms[N * MP];
  __shared__ float Rs[N * HP];  // R[:, 32 oj .. + 32]
  __shared__ float Ys[N * HP];  // Y = Mx R_oj
  __shared__ float Ls[N * (W + 4)];
  const int q = blockIdx.x >> 1, j = blockIdx.x & 1, oj = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* Rg = T1 + (size_t)(j == 0 ? 2 * q + 1 : 2 * q) * N * N + W + 32 * oj;
  const double* Lg = T1 + (size_t)(j == 0 ? 2 * q : 2 * q + 1) * N * N;
  // 16-byte loads, all issued before the first use (latency-bound otherwise)
#pragma unroll
  for (int u = 0; u < N * 32 / 2 / kUpdThreads; ++u) {
    const int idx = u * kUpdThreads + tid, r = idx >> 4, cc = (idx & 15) * 2;
    const double2 v = *reinterpret_cast<const double2*>(Rg + (size_t)r * N + cc);
    Rs[r * HP + cc] = (float)v.x;
    Rs[r * HP + cc + 1] = (float)v.y;
  }
#pragma unroll
  for (int u = 0; u < N * W / 2 / kUpdThreads; ++u) {
    const int idx = u * kUpdThreads + tid, r = idx >> 5, cc = (idx & 31) * 2;
    const double2 v = *reinterpret_cast<const double2*>(Lg + (size_t)r * N + cc);
    Ls[r * (W + 4) + cc] = (float)v.x;
    Ls[r * (W + 4) + cc + 1] = (float)v.y;
  }
  // slabs of quad q: r = 0 (a,d), 1 (b,c), 2 (a,b), 3 (c,d), gch chunks each
  // (16-byte loads, four independent sums per thread and four slabs' worth in
  // flight: the one-float loop was load-latency bound, 94 us per 128-pair quad
  // step at 83 % wait-any, profiles/r5_prof)
  const float* base = slabs + (size_t)q * 4 * gch * W * W;
  constexpr int E4 = W * W / 4;
#pragma unroll 4
  for (int idx = tid; idx < 4 * E4; idx += kUpdThreads) {
    const int r = idx / E4, e4 = idx % E4, i = (4 * e4) / W, jj = (4 * e4) % W;
    const auto sv = slab_sum<0>(base + (size_t)r * gch * W * W, 4 * e4, W * W, gch);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ju = jj + u;
      const int row = r == 0 ? i : r == 1 ? W + ju : r == 2 ? i : W + i;
      const int col = r == 0 ? W + ju : r == 1 ? i : r == 2 ? ju : W + ju;
      Ms[row * MP + col] = (float)sv[u];
    }
  }
  __syncthreads();
  const int li = lane & 31, lk = lane >> 5;
  if (wave < 4) {  // Y = Mx R_oj (N x 32): wave w owns row tile w
    M::acc_t acc = M::zero();
    const int i = wave * 32 + li;
#pragma unroll 8
    for (int l0 = 0; l0 < N; l0 += 2) {
      const int l = l0 + lk;
      const float av = j == 0 ? Ms[i * MP + l] : Ms[l * MP + i];
      acc = M::mfma(av, Rs[l * HP + li], acc);
    }
#pragma unroll
    for (int e = 0; e < M::NACC; ++e) Ys[(wave * 32 + M::acc_row(e, lane)) * HP + li] = acc[e];
  }
  __syncthreads();
  if (wave < 2) {  // out[:, 32 oj ..] = Lx^T Y (W x 32): wave w owns row tile w
    M::acc_t acc = M::zero();
#pragma unroll 8
    for (int k0 = 0; k0 < N; k0 += 2) {
      const int k = k0 + lk;
      acc = M::mfma(Ls[k * (W + 4) + wave * 32 + li], Ys[k * HP + li], acc);
    }
    float* out = upd + (size_t)blockIdx.x * W * W;
#pragma unroll
    for (int e = 0; e < M::NACC; ++e)
      out[(wave * 32 + M::acc_row(e, lane)) * W + 32 * oj + li] = acc[e];
  }
}

// [a b c d] <- [a b c d] T, T-STATIONARY (round 5; 16x16x32 MFMAs round 6).
// The round-4 apply streamed the 384 KB split T through LDS for every 128-row
// tile (3.2 GB of T per 64-pair quad step against 2.1 GB of data; 1.71 ms per
// 128-pair quad step, profiles/r4_quad).  Here a workgroup keeps T in
// REGISTERS for thousands of rows:
//   * 8 waves (two per SIMD), wave w owns output column tile w (32 of the
//     quad's 256 columns, two 16-column sub-tiles) and holds its split T - I
//     slice, 8 k blocks of 32 x 2 sub-tiles x NP bf16x8 = 192 VGPRs for
//     NP = 3, for the whole launch;
//   * the workgroup walks a contiguous range of 32-row tiles of A then V
//     (every tile all 256 columns: it owns its rows, so in place is safe);
//   * each wave LDS-DMAs (global_load_lds_dwordx4) its own 32 columns of the
//     tile two tiles ahead into a wave-private raw image (no VGPRs in
//     flight), splits them -- exactly k block w -- into the shared B-fragment
//     image of the tile (double-buffered, one barrier per tile), runs 8 k
//     blocks x 2 x 2 sub-tiles x (1 + 5) v_mfma_f32_16x16x32_bf16 (leading
//     product and the small ones in two accumulators, as apply_split_kernel),
//     and reads its own raw values for the delta-form epilogue
//     Y = X + X (T - I) back from its raw image.
// MFMA shape (round 6): the kernel is power-limited -- the dense form runs at
// 1.77 GHz with its matrix pipe 61 % busy at that clock, without global
// memory at 2.10 GHz, memory alone at 2.45 GHz (profiles/r6_clock) -- and the
// 16x16x32 bf16 MFMA holds a higher clock than 32x32x16 for the same flops
// (MI355X_MICROARCH "DVFS give-back" (7)); same cycles, registers and LDS
// reads per flop.
// (The raw image is plain [col][row]: the split's and epilogue's dword reads
// meet 2-way bank conflicts, which cost less than the registers a swizzle's
// extra lane offsets took from the T slice.)
// Work: the active quads (some step-s or step-(s+1) pair rotated) are listed
// by every wave with ballots over the skip flags (no extra launch, no host
// sync); their tiles, flattened, are dealt to the persistent grid in
// contiguous ranges of equal cost (one workgroup per CU: the LDS is 160 KB).
// Inside a quad, what T leaves unchanged is skipped (SPARSE in the kernel).
constexpr int kQuadTsThreads = 512;
constexpr int kQuadTsGrid = 256;
// While the other chain's latency-bound kernels (Gram, EVDs, Q builds, update)
// run concurrently on another stream (two-chain issue, every multi-GPU plan),
// a smaller grid leaves them CUs to start on at once instead of behind the
// persistent apply's 160 KB-LDS workgroups.  16384^2 rank plans, ms per sweep
// (profiles/r6_grid): P = 4 (8 quads per apply) 256 WGs 65.5-69.8, 224
// 64.6-65.3, 208 63.8-65.6, 192 63.4-64.1; P = 2 (16 quads) 256 118.0-125.5,
// 224 116.4-118.3, 192 118.4-120.7.  The merged one-GPU issue keeps the
// whole chip.
__host__ __device__ constexpr int quad_ts_grid_shared(int nq) { return nq <= 8 ? 192 : 224; }
template <int NP>
struct QuadTsLds {
  static constexpr int S_BYTES = 16 * NP * SVDJ_WAVE * 16;  // split image of a 32-row tile
  static constexpr int R_BYTES = 8 * 32 * 32 * 4;           // raw tile, wave w at 4 KB * w: [col][row]
  static constexpr int TOTAL = 2 * S_BYTES + 2 * R_BYTES;
};
static_assert(QuadTsLds<3>::TOTAL <= 163840, "T-stationary quad apply LDS");

// s_waitcnt vmcnt(n rounded down to even), n <= 20 (wave-uniform n)
__device__ __forceinline__ void wait_vmcnt_upto(int n) {
  switch (n >> 1) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
  }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
}

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ABL (tools/micro/quad_apply_ab.hip only; production launches ABL = 0):
// bit 0 one MFMA per k block and sub-tile instead of 1 + (products of order
// < NP), B fragments still read; bit 1 no global memory (no DMA, no waits, no
// stores); bit 2 no MFMA loop at all (split, barrier, epilogue, DMA only);
// bit 3 never the cheap (first-order) k-block form.
template <int NP, int ABL = 0>
__global__ __launch_bounds__(kQuadTsThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void
apply_quad_ts_kernel(float* __restrict__ A, int lda, int a_tiles, float* __restrict__ V, int ldv,
                     int v_tiles, const int32_t* __restrict__ pairs, int nq,
                     const bf16x8* __restrict__ Ts, const int32_t* __restrict__ skip1,
                     const int32_t* __restrict__ skip2, uint32_t* __restrict__ work = nullptr,
                     float cheap_tol = 0.0078125f) {
  using L = QuadTsLds<NP>;
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i16 = lane & 15, g = lane >> 4;
  auto active = [&](int q) -> bool {  // all four flags loaded (no short-circuit branches)
    if (q >= nq) return false;
    return (skip1[2 * q] & skip1[2 * q + 1] & skip2[2 * q] & skip2[2 * q + 1]) == 0;
  };
  // Cost of a quad's tile, 1 .. 4: the column blocks of [a b c d] its flags say
  // can change (a: (a,c) or (a,d) rotated, b: (b,d) or (b,c), c: (a,c) or
  // (b,c), d: (b,d) or (a,d)) -- about the blocks the tile moves, see SPARSE
  // below.  Only the deal uses it: what is skipped is decided from T's values.
  auto cost = [&](int q) -> int {
    if (q >= nq) return 1;
    const int ac = skip1[2 * q] == 0, bd = skip1[2 * q + 1] == 0;
    const int ad = skip2[2 * q] == 0, bc = skip2[2 * q + 1] == 0;
    const int w = (ac | ad) + (bd | bc) + (ac | bc) + (bd | ad);
    return w < 1 ? 1 : w;
  };
  const unsigned long long below = (1ull << lane) - 1ull;
  int nact = 0, wsum = 0;
  for (int b0 = 0; b0 < nq; b0 += SVDJ_WAVE) {
    const bool a = active(b0 + lane);
    const int w1 = cost(b0 + lane) - 1;
    const int n = __popcll(__ballot(a));
    nact += n;
    wsum += n + __popcll(__ballot(a && (w1 & 1))) + 2 * __popcll(__ballot(a && (w1 & 2)));
  }
  if (nact == 0) return;
  const int G = (int)gridDim.x, nt = a_tiles + v_tiles;
  // The active quads' tiles, flattened quad-major, are dealt to the grid in
  // contiguous ranges of equal COST (a range may span quads: one more
  // T-slice load).  Round 5 split each quad into G / nact equal slices, which left
  // G mod nact workgroups idle -- up to a quarter of the grid (52 active
  // quads: 208 of 256 busy) once quads start to skip; equal tile counts leave
  // the workgroups that hold fully rotated quads to finish last once the
  // others skip blocks.  bound(p): the tile position (quad-major) at cost
  // offset p, the same function in every workgroup and monotone in p; with
  // equal costs it is the equal-count deal p / cost.
  const long long wtotal = (long long)wsum * nt;
  auto bound = [&](long long p) -> long long {
    if (p >= wtotal) return (long long)nact * nt;
    int rq = 0, rt = 0;
    for (int b0 = 0, seenq = 0, seenw = 0; b0 < nq; b0 += SVDJ_WAVE) {
      const bool a = active(b0 + lane);
      const int w = cost(b0 + lane), w1 = w - 1;
      const unsigned long long ma = __ballot(a), m0 = __ballot(a && (w1 & 1)),
                               m1 = __ballot(a && (w1 & 2));
      const int myq = seenq + __popcll(ma & below);
      const long long lo = (long long)(seenw + __popcll(ma & below) + __popcll(m0 & below) +
                                       2 * __popcll(m1 & below)) * nt;
      const unsigned long long hit = __ballot(a && p >= lo && p < lo + (long long)w * nt);
      if (hit) {
        const int src_lane = __ffsll((long long)hit) - 1;
        rq = __shfl(myq, src_lane);
        rt = __shfl((int)((p - lo) / w), src_lane);
      }
      seenq += __popcll(ma);
      seenw += __popcll(ma) + __popcll(m0) + 2 * __popcll(m1);
    }
    return (long long)__builtin_amdgcn_readfirstlane(rq) * nt + __builtin_amdgcn_readfirstlane(rt);
  };
  const long long g_end = bound((long long)(blockIdx.x + 1) * wtotal / G);
  for (long long pos = bound((long long)blockIdx.x * wtotal / G); pos < g_end;) {
    const int qi = (int)(pos / nt);
    const int t0 = (int)(pos % nt);
    const int t1 = (int)((long long)t0 + (g_end - pos) < nt ? (long long)t0 + (g_end - pos) : nt);
    pos += t1 - t0;
    int q = 0;
    for (int b0 = 0, seen = 0; b0 < nq; b0 += SVDJ_WAVE) {  // the qi-th active quad
      const bool a = active(b0 + lane);
      const unsigned long long m = __ballot(a);
      const int cnt = __popcll(m);
      if (seen <= qi && qi < seen + cnt) {
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        q = b0 + __ffsll((long long)__ballot(a && pre == qi - seen)) - 1;
      }
      seen += cnt;
    }
    q = __builtin_amdgcn_readfirstlane(q);
    // this wave's split T - I slice: Ts[q][kb][ct = wave][cs][part][lane]
    bf16x8 qf[8][2][NP];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
      for (int cs = 0; cs < 2; ++cs) {
        const bf16x8* tp = Ts + ts_frag(q, kb, wave, cs, NP) + lane;
#pragma unroll
        for (int p = 0; p < NP; ++p) qf[kb][cs][p] = tp[p * SVDJ_WAVE];
      }
    // Halves of the k range (k blocks 0-3 = blocks a, b of the quad, 4-7 =
    // c, d) whose slice of T - I is below cheap_tol = 2^-7 in magnitude: there
    // the order-2 products (q0 x2, q1 x1, q2 x0 <= 3 2^-18 |t||x| <= 3 2^-25
    // |x| per term, at the fp32 rounding of the output) are dropped, 3 MFMAs
    // per k block and sub-tile instead of 6.  Round 5 used 2^-9; 2^-7 and
    // 2^-6 measured 16384^2 -27 / -45 ms with residual 1.141 -> 1.151 / 1.173
    // e-5 and the same orthogonality (profiles/r6_issue); 2^-7 kept.  With T = T1 T2 (pairs (a,c), (b,d) then
    // (a,d), (b,c)), for an output column in a or b the rows of a and b are
    // second order in the rotation angles (T_aa - I, T_ba = T1_bd T2_da),
    // those of c and d first order; for c or d the other way round -- so once
    // the angles are below ~0.04 one half of every column tile takes the
    // cheap form.
    uint32_t cheap = 0;
    if constexpr (NP == 3 && (ABL & 8) == 0) {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        float mx = 0.0f;
#pragma unroll
        for (int kb = 4 * hf; kb < 4 * hf + 4; ++kb)
#pragma unroll
          for (int cs = 0; cs < 2; ++cs)
#pragma unroll
            for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf((float)qf[kb][cs][0][e]));
        if (wave_max(mx) <= cheap_tol) cheap |= 1u << hf;
      }
      cheap = __builtin_amdgcn_readfirstlane(cheap);
    }
    // SPARSE: what T leaves unchanged is neither computed nor moved.  T is
    // the identity plus the pairs' plane rotations: a pair that did not
    // rotate contributes an exact identity block (qbuild_quad_kernel, ns = 0),
    // so late in a solve most of T - I is exactly zero.  From the values of
    // the slice (all parts; a sign bit alone is a zero), never from the flags:
    //   chg  : bit c set when column c of the wave's 32 has a nonzero column in
    //          T - I: the columns the apply changes.  Others are not stored,
    //          and with chg == 0 the wave runs no MFMA, epilogue or store.
    //   nzkb : bit kb set when k block kb (source columns 32 kb .. + 31 of the
    //          quad, the ones wave kb loads and splits) is nonzero in this
    //          slice; a zero one is skipped in the MFMA loop.
    //   src  : the OR of every wave's nzkb (8 words of split image 1 and one
    //          barrier per item): bit w set when wave w's columns feed some
    //          wave's product.  A wave with chg == 0 and bit `wave` of src
    //          clear issues no DMA and no split for the item.
    // INVARIANT: split skipped by wave w  =>  bit w of src clear  =>  k block w
    // is zero in every wave's slice  =>  every wave skips it: the stale
    // fragments (any bit pattern, NaNs included) are never multiplied, not
    // even by zero.  Every skipped operation contributed an exact zero, so the
    // results are those of the dense form, but for the sign of a zero: an
    // untouched -0.0, which x + 0 used to rewrite as +0.0, is now kept.
    // Every wave reaches every barrier whatever it skips.
    uint32_t chg = 0, nzkb = 0;
    {
      using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
      uint32_t cnz[2] = {0u, 0u};
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) {
        uint32_t ko = 0;
#pragma unroll
        for (int cs = 0; cs < 2; ++cs) {
          uint32_t o = 0;
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            const u32x4 d = __builtin_bit_cast(u32x4, qf[kb][cs][p]);
            o |= d[0] | d[1] | d[2] | d[3];
          }
          cnz[cs] |= o;
          ko |= o;
        }
        if (__ballot((ko & 0x7fff7fffu) != 0)) nzkb |= 1u << kb;
      }
#pragma unroll
      for (int cs = 0; cs < 2; ++cs) {  // lane 16 g + i holds rows of column 16 cs + i
        const unsigned long long m = __ballot((cnz[cs] & 0x7fff7fffu) != 0);
        chg |= (uint32_t)((m | m >> 16 | m >> 32 | m >> 48) & 0xffffull) << (16 * cs);
      }
      chg = __builtin_amdgcn_readfirstlane(chg);
      nzkb = __builtin_amdgcn_readfirstlane(nzkb);
    }
    // products per tile in quarter units (word 6 counts one unit per cheap
    // half and two per full half of 4 k blocks)
    uint32_t qunits = 0;
    if (chg != 0) {
#pragma unroll
      for (int kb = 0; kb < 8; ++kb)
        if ((nzkb >> kb) & 1u) qunits += NP == 3 && ((cheap >> (kb >> 2)) & 1u) == 0 ? 2u : 1u;
    }
    uint32_t src = 0, qsum = 0;
    {
      uint32_t* xw = reinterpret_cast<uint32_t*>(lds + L::S_BYTES);
      if (lane == 0) xw[wave] = nzkb | qunits << 8;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        const uint32_t v = xw[w];
        src |= v & 0xffu;
        qsum += v >> 8;
      }
      src = __builtin_amdgcn_readfirstlane(src);
      qsum = __builtin_amdgcn_readfirstlane(qsum);
    }
    const bool loads = chg != 0 || ((src >> wave) & 1u) != 0;
    // store instruction (cs, e) writes columns 16 cs + e + 4 g: issued when one
    // of them changes, each lane storing its own column only if it does
    const uint32_t cset = (chg | chg >> 4 | chg >> 8 | chg >> 12) & 0x000f000fu;
    const int nst = 2 * __popc(cset);  // store instructions per tile, at least
    const uint32_t lchg = chg >> (4 * g);
    // this wave's 32 columns: block wave >> 1 of [a b c d], half wave & 1
    const int32_t* qp = pairs + 4 * q;
    const int qb = wave >> 1;
    const int col0 = __builtin_amdgcn_readfirstlane(qp[(qb & 1) * 2 + (qb >> 1)] * 64 + (wave & 1) * 32);
    float* const ownA = A + (size_t)col0 * lda;
    float* const ownV = V ? V + (size_t)col0 * ldv : nullptr;

    // raw tile t, own 32 columns -> R[buf] (4 x 1 KB): lane -> column
    // 8i + lane / 8, row chunk lane % 8 (one 32-bit lane offset from a
    // wave-uniform column base)
    auto dma = [&](int t, int buf) {
      if constexpr ((ABL & 2) != 0) return;
      const bool isA = t < a_tiles;
      const float* base = isA ? ownA : ownV;
      const int ld = isA ? lda : ldv, r0 = (isA ? t : t - a_tiles) * 32;
      char* dst = lds + 2 * L::S_BYTES + buf * L::R_BYTES + wave * 4096;
      const uint32_t o = (uint32_t)((lane >> 3) * ld + (lane & 7) * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(&at_u32(base + (size_t)(8 * i) * ld + r0, o), dst + i * 1024,
                                         16, 0, 0);
    };
    // lane bases into the raw image [col][row]: split reads (column 8g + e,
    // row 16 rs + i) and epilogue reads (column 16 cs + 4g + e, row 16 rs + i)
    const int sb = 256 * g + i16, eb = 128 * g + i16;
    auto tile = [&](int t, auto bufc, auto chc) {
      constexpr int buf = decltype(bufc)::value;
      constexpr int CH = decltype(chc)::value;  // cheap halves (bit 0: k blocks 0-3, bit 1: 4-7)
      // 1. own DMA of tile t landed (younger: stores of t-1, DMA of t+1)
      //    counted from what this wave issues: nst stores, or more (a count
      //    that is too small only waits longer)
      const int younger = (t > t0 ? nst : 0) + (t + 1 < t1 ? 4 : 0);
      if constexpr ((ABL & 2) != 0) (void)younger;
      else wait_vmcnt_upto(younger);
      const float* R = reinterpret_cast<const float*>(lds + 2 * L::S_BYTES + buf * L::R_BYTES + wave * 4096);
      // 2. split own columns (k block `wave`) into the shared B-fragment image
      //    S[buf]: [kb][rs][part][lane (i, g)] element e = X[16 rs + i][32 kb + 8g + e]
      {
        bf16x8* Sw = reinterpret_cast<bf16x8*>(lds + buf * L::S_BYTES) + lane;
#pragma unroll
        for (int rs = 0; rs < 2; ++rs) {
          bf16x8 parts[NP];
          float xv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) xv[e] = R[sb + 32 * e + 16 * rs];
          split_bf16x8<NP>(xv, parts);
#pragma unroll
          for (int i = 0; i < NP; ++i) Sw[((2 * wave + rs) * NP + i) * SVDJ_WAVE] = parts[i];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // 3. per 16-row half rs of the tile: 8 k blocks x 2 column sub-tiles x
      //    (1 + 5) MFMAs (1 + 2 in a cheap half) against the register-resident
      //    slice, then that half's epilogue (one half's accumulators live at a
      //    time: 16 VGPRs, what lets the T slice stay in registers)
      const bf16x8* Sr = reinterpret_cast<const bf16x8*>(lds + buf * L::S_BYTES) + lane;
      const bool isA = t < a_tiles;
      float* const own = isA ? ownA : ownV;
      const int ld = isA ? lda : ldv, r0 = (isA ? t : t - a_tiles) * 32;
      const uint32_t st_off = (uint32_t)(4 * g * ld + i16) + (uint32_t)r0;
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        f32x4 acc[2], lo[2];
#pragma unroll
        for (int cs = 0; cs < 2; ++cs)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[cs][e] = lo[cs][e] = 0.0f;
        auto khalf = [&](auto k0c) {
          constexpr int k0 = decltype(k0c)::value;
#pragma unroll
          for (int kb = k0; kb < k0 + 4; ++kb) {
            // a k block that is zero in this slice (SPARSE: its fragments may be stale)
            if (((nzkb >> kb) & 1u) == 0) continue;
            bf16x8 xs[NP];
            if constexpr ((ABL & 1) != 0) {
              using i32x4 = __attribute__((ext_vector_type(4))) int;
              i32x4 x = __builtin_bit_cast(i32x4, Sr[((kb * 2 + rs) * NP) * SVDJ_WAVE]);
#pragma unroll
              for (int i = 1; i < NP; ++i)
                x ^= __builtin_bit_cast(i32x4, Sr[((kb * 2 + rs) * NP + i) * SVDJ_WAVE]);
#pragma unroll
              for (int cs = 0; cs < 2; ++cs) acc[cs] = mfma16(qf[kb][cs][0], __builtin_bit_cast(bf16x8, x), acc[cs]);
            } else if constexpr (NP == 3 && ((CH >> (k0 / 4)) & 1) != 0) {
              xs[0] = Sr[((kb * 2 + rs) * NP + 0) * SVDJ_WAVE];
              xs[1] = Sr[((kb * 2 + rs) * NP + 1) * SVDJ_WAVE];
#pragma unroll
              for (int cs = 0; cs < 2; ++cs) {
                lo[cs] = mfma16(qf[kb][cs][0], xs[1], lo[cs]);
                lo[cs] = mfma16(qf[kb][cs][1], xs[0], lo[cs]);
                acc[cs] = mfma16(qf[kb][cs][0], xs[0], acc[cs]);
              }
            } else {
#pragma unroll
              for (int i = 0; i < NP; ++i) xs[i] = Sr[((kb * 2 + rs) * NP + i) * SVDJ_WAVE];
#pragma unroll
              for (int cs = 0; cs < 2; ++cs) {
#pragma unroll
                for (int ord = NP - 1; ord >= 1; --ord)  // products of order ord, small first
#pragma unroll
                  for (int a = 0; a <= ord; ++a) lo[cs] = mfma16(qf[kb][cs][a], xs[ord - a], lo[cs]);
                acc[cs] = mfma16(qf[kb][cs][0], xs[0], acc[cs]);
              }
            }
            // no scheduling across k blocks: hoisted fragment loads of later
            // blocks pushed the T slice out of registers
            __builtin_amdgcn_sched_barrier(0);
          }
        };
        if constexpr ((ABL & 4) == 0) {
          khalf(std::integral_constant<int, 0>{});
          khalf(std::integral_constant<int, 4>{});
        }
        // 4. own raw values of this half, still in this wave's raw image R[buf]
        //    (its refill, tile t + 2, is issued below), and the delta-form
        //    store, in place (acc[cs] register e is own column 16 cs + 4g + e,
        //    row 16 rs + i).  (Staging the finished tile
        //    through R[buf] for 16-byte stores cut the compute-only time of the
        //    32x32x16 form 1229 -> 1037 us but not the solve's:
        //    profiles/r6_apply/ablation_vector_epilogue_rejected.jsonl.)
        //    Only changed columns are stored (SPARSE); all 32 changed is the
        //    unpredicated form.
        if (chg == 0xffffffffu) {
#pragma unroll
          for (int cs = 0; cs < 2; ++cs) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = R[eb + 512 * cs + 32 * e + 16 * rs];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float y = v[e] + (acc[cs][e] + lo[cs][e]);
              if ((ABL & 2) == 0 || y == -1.2345e-30f)
                at_u32(own + (size_t)(16 * cs + e) * ld + 16 * rs, st_off) = y;
            }
          }
        } else {
#pragma unroll
          for (int cs = 0; cs < 2; ++cs) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = R[eb + 512 * cs + 32 * e + 16 * rs];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float y = v[e] + (acc[cs][e] + lo[cs][e]);
              if (((cset >> (16 * cs + e)) & 1u) != 0 && ((lchg >> (16 * cs + e)) & 1u) != 0 &&
                  ((ABL & 2) == 0 || y == -1.2345e-30f))
                at_u32(own + (size_t)(16 * cs + e) * ld + 16 * rs, st_off) = y;
            }
          }
        }
      }
      // 5. tile t + 2 into the raw image this wave just consumed
      if (t + 2 < t1) dma(t + 2, buf);
    };
    if (loads) {
      if (t0 < t1) dma(t0, 0);
      if (t0 + 1 < t1) dma(t0 + 1, 1);
    }
    // the tile loop specialised per cheap-half mask (a branch per k half
    // inside one loop made the compiler spill the T slice)
    auto run = [&](auto chc) {
      for (int t = t0; t < t1; t += 2) {
        tile(t, std::integral_constant<int, 0>{}, chc);
        if (t + 1 < t1) tile(t + 1, std::integral_constant<int, 1>{}, chc);
      }
    };
    if (chg == 0) {
      // nothing of this wave's changes (SPARSE): it feeds the others -- load
      // and split as in tile() -- or only keeps the barriers
      for (int t = t0; t < t1; ++t) {
        const int buf = (t - t0) & 1;
        if (loads) {
          if constexpr ((ABL & 2) == 0) wait_vmcnt_upto(t + 1 < t1 ? 4 : 0);
          const float* R = reinterpret_cast<const float*>(lds + 2 * L::S_BYTES + buf * L::R_BYTES + wave * 4096);
          bf16x8* Sw = reinterpret_cast<bf16x8*>(lds + buf * L::S_BYTES) + lane;
#pragma unroll
          for (int rs = 0; rs < 2; ++rs) {
            bf16x8 parts[NP];
            float xv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] = R[sb + 32 * e + 16 * rs];
            split_bf16x8<NP>(xv, parts);
#pragma unroll
            for (int i = 0; i < NP; ++i) Sw[((2 * wave + rs) * NP + i) * SVDJ_WAVE] = parts[i];
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (loads && t + 2 < t1) dma(t + 2, buf);
      }
    } else if (cheap == 0) run(std::integral_constant<int, 0>{});
    else if constexpr (NP == 3) {
      if (cheap == 1) run(std::integral_constant<int, 1>{});
      else if (cheap == 2) run(std::integral_constant<int, 2>{});
      else run(std::integral_constant<int, 3>{});
    }
    // work counters of the sweep (metric words 6, 7; svdj_stop.h): MFMAs the
    // waves issued in 32x32x16 units of 24 (per wave 96, 72 or 48 per tile =
    // twice as many 16x16x32 ones; a skipped k block or wave adds nothing, the
    // quarter units of the item's eight waves summed and rounded down once:
    // less than one unit per item lost), and tiles of active quads walked
    if (work && lane == 0 && wave == 0) {
      atomicAdd(&work[0], (uint32_t)(t1 - t0) * qsum >> 2);
      atomicAdd(&work[1], (uint32_t)(t1 - t0));
    }
    // the next item re-stages both images
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
}

// The six cross Grams of a quad step, every block read ONCE (round 5).  The
// round-4 form computed them as 3P independent f32-MFMA slabs, each reading
// its two blocks: every block of a quad was read three times and the f32
// MFMAs (1/16 of the bf16 rate) set the pace (722 us per 128-pair quad step
// vs 2 x 215 us for the two single-step Grams it replaces).  Here
// one workgroup (8 waves) per (quad, row chunk):
//   * wave w LDS-DMAs column tile w (32 of the quad's 256 columns, [a b c d]
//     order) of each 32-row slab two slabs ahead into a wave-private raw
//     image, and splits it into 3 RNE bf16 parts -- lane (i, g) of 16-column
//     sub-tile s: column 16 s + i, rows 8g .. 8g+7, exactly the A and the B
//     operand of v_mfma_f32_16x16x32_bf16 -- kept in registers and written to
//     the shared fragment image for the other waves;
//   * OWNER-based tiles (round 6): the 24 needed 32 x 32 output tiles are the
//     pairs of column tiles from different blocks; each is computed by one
//     of its two column tiles' waves (kGramPartner: every wave 3 partners), so
//     a wave's own operand never leaves its registers and it reads only its 3
//     partners' fragments (18 x 1 KB per slab and wave instead of 36: the
//     round-5 form, any 3 tiles per wave with both operands from LDS, was
//     LDS-bandwidth bound -- 142 us of 278 with one MFMA per product,
//     profiles/r6_apply/ablation_gram.jsonl);
//   * each 16 x 16 sub-tile takes the 6 products of order < 3 (leading product
//     and the small ones in two accumulators), the error of a product below
//     2^-26 relative, like the split apply;
//   * the tiles go straight to the slab layout the consumers read: slab
//     (pair 2q) = C_ac, (2q+1) = C_bd, then per quad C_ad, C_bc, C_ab, C_cd
//     (the order quad_update_kernel reads), one W x W slab per row chunk; a
//     tile whose owner is its slab's column block is stored transposed.
constexpr int kGramQThreads = 512;
template <int NP>
struct GramQLds {
  static constexpr int S_BYTES = 8 * 2 * NP * SVDJ_WAVE * 16;  // 8 col tiles x 2 sub-tiles x NP parts
  static constexpr int R_BYTES = 8 * 32 * 32 * 4;              // raw 32-row slab, wave w at 4 KB * w
  static constexpr int TOTAL = 2 * S_BYTES + 2 * R_BYTES;
};
static_assert(GramQLds<3>::TOTAL <= 163840, "quad Gram LDS");
// Partners of column tile w (tile t is block t >> 1 of [a b c d], half t & 1):
// the 24 pairs of tiles from different blocks, each listed once, 3 per tile
// (3 bits each, partner j at bits 3j).
constexpr int kGramPartners[8] = {2 | 3 << 3 | 4 << 6, 2 | 3 << 3 | 5 << 6, 4 | 5 << 3 | 6 << 6,
                                  4 | 5 << 3 | 7 << 6, 1 | 6 << 3 | 7 << 6, 0 | 6 << 3 | 7 << 6,
                                  0 | 1 << 3 | 3 << 6, 0 | 1 << 3 | 2 << 6};
// every unordered pair of tiles from different blocks exactly once, none within a block
constexpr bool gram_partners_cover() {
  int seen[8][8] = {};
  for (int w = 0; w < 8; ++w)
    for (int j = 0; j < 3; ++j) {
      const int y = kGramPartners[w] >> (3 * j) & 7;
      if ((y >> 1) == (w >> 1)) return false;
      ++seen[w < y ? w : y][w < y ? y : w];
    }
  for (int x = 0; x < 8; ++x)
    for (int y = x + 1; y < 8; ++y)
      if (seen[x][y] != ((x >> 1) != (y >> 1) ? 1 : 0)) return false;
  return true;
}
static_assert(gram_partners_cover(), "quad Gram partner table");
__device__ __forceinline__ int gram_partners(int w) {
  int r = kGramPartners[0];
#pragma unroll
  for (int t = 1; t < 8; ++t) r = w == t ? kGramPartners[t] : r;
  return r;
}
// Product (slab) of blocks (x, y) of [a b c d]: ac bd ad bc ab cd = 0 .. 5;
// bit 3 set when (x, y) is the transposed order.
__host__ __device__ constexpr int gram_product_fwd(int x, int y) {
  return x == 0 && y == 2 ? 0 : x == 1 && y == 3 ? 1 : x == 0 && y == 3 ? 2 : x == 1 && y == 2 ? 3
       : x == 0 && y == 1 ? 4 : x == 2 && y == 3 ? 5 : -1;
}
__host__ __device__ constexpr int gram_product(int x, int y) {
  return gram_product_fwd(x, y) >= 0 ? gram_product_fwd(x, y) : 8 | gram_product_fwd(y, x);
}
static_assert(gram_product(2, 0) == 8 && gram_product(3, 2) == 13, "gram_product");
// ABL (tools/micro/quad_apply_ab.hip only; production launches ABL = 0):
// bit 0 one MFMA per output sub-tile and slab instead of 6; bit 1 no global
// reads (no DMA, no waits).
// NP = 2 (sweeps far from convergence, see launch_quad_gram_evd): 2 bf16
// parts and the 3 products of order < 2 -- couplings to ~2^-17 |x||y|,
// which only steers the rotation angles (T stays orthogonal to fp64).
template <int ABL = 0, int NP = 3>
__global__ __launch_bounds__(kGramQThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void
gram_quad_kernel(const float* __restrict__ A, int lda, int m_pad, const int32_t* __restrict__ pairs,
                 int P, int rows_per_chunk, float* __restrict__ slabs) {
  constexpr int W = 64;
  using L = GramQLds<NP>;
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const int q = blockIdx.x, chunk = blockIdx.y, nchunk = gridDim.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i16 = lane & 15, g = lane >> 4;
  const int32_t* qp = pairs + 4 * q;  // (a, c), (b, d)
  auto blk = [&](int qb) { return qp[(qb & 1) * 2 + (qb >> 1)]; };  // [a b c d] -> block id
  const int r_begin = chunk * rows_per_chunk;
  const int r_end = min(m_pad, r_begin + rows_per_chunk);
  const int ns = (r_end - r_begin) / 32;  // rows_per_chunk and m_pad are multiples of 128
  const float* own = A + (size_t)__builtin_amdgcn_readfirstlane(blk(wave >> 1) * W + (wave & 1) * 32) * lda;
  const int pk = __builtin_amdgcn_readfirstlane(gram_partners(wave));
  // raw image [col][16-byte row chunk], chunk slot j of column col holding
  // rows 4 (j ^ (col & 7)) .. + 3: the split's reads (8 rows of one column per
  // lane, lanes at a 128-byte column stride) then spread over the banks
  // instead of piling onto a few (35 % bank-conflict cycles unswizzled)
  auto dma = [&](int sl, int buf) {
    if constexpr ((ABL & 2) != 0) return;
    const int r0 = r_begin + 32 * sl;
    char* dst = lds + 2 * L::S_BYTES + buf * L::R_BYTES + wave * 4096;
    const int jr = ((lane & 7) ^ (lane >> 3)) * 4;  // col & 7 == lane >> 3 for every i
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds(own + (size_t)(8 * i + (lane >> 3)) * lda + r0 + jr,
                                       dst + i * 1024, 16, 0, 0);
  };
  // [partner j][own sub-tile s][partner sub-tile s2]
  f32x4 acc[3][2][2], lo[3][2][2];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][s][s2][e] = lo[j][s][s2][e] = 0.0f;
  auto slab = [&](int sl, auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    if constexpr ((ABL & 2) != 0) {
    } else if (sl + 1 < ns) wait_vmcnt<4>();
    else wait_vmcnt<0>();
    bf16x8 xf[2][NP];
    {  // split own column tile: sub-tile s, column 16 s + i, rows 8g .. 8g+7
      const float* R = reinterpret_cast<const float*>(lds + 2 * L::S_BYTES + buf * L::R_BYTES + wave * 4096);
      bf16x8* Sw = reinterpret_cast<bf16x8*>(lds + buf * L::S_BYTES) + lane;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int c = 16 * s + i16;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(R + c * 32 + 4 * ((2 * g) ^ (c & 7)));
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(R + c * 32 + 4 * ((2 * g + 1) ^ (c & 7)));
        const float xv[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        split_bf16x8<NP>(xv, xf[s]);
#pragma unroll
        for (int i = 0; i < NP; ++i) Sw[((wave * 2 + s) * NP + i) * SVDJ_WAVE] = xf[s][i];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bf16x8* Sr = reinterpret_cast<const bf16x8*>(lds + buf * L::S_BYTES) + lane;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int yt = (pk >> (3 * j)) & 7;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 yf[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) yf[i] = Sr[((yt * 2 + s2) * NP + i) * SVDJ_WAVE];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if constexpr ((ABL & 1) != 0) {
            using i32x4 = __attribute__((ext_vector_type(4))) int;
            i32x4 yy = __builtin_bit_cast(i32x4, yf[0]);
#pragma unroll
            for (int i = 1; i < NP; ++i) yy ^= __builtin_bit_cast(i32x4, yf[i]);
            acc[j][s][s2] = mfma16(xf[s][0], __builtin_bit_cast(bf16x8, yy), acc[j][s][s2]);
          } else {
#pragma unroll
            for (int ord = NP - 1; ord >= 1; --ord)  // products of order ord, small first
#pragma unroll
              for (int a = 0; a <= ord; ++a) lo[j][s][s2] = mfma16(xf[s][a], yf[ord - a], lo[j][s][s2]);
            acc[j][s][s2] = mfma16(xf[s][0], yf[0], acc[j][s][s2]);
          }
        }
      }
    }
    if (sl + 2 < ns) dma(sl + 2, buf);
  };
  if (ns > 0) dma(0, 0);
  if (ns > 1) dma(1, 1);
  for (int sl = 0; sl < ns; sl += 2) {
    slab(sl, std::integral_constant<int, 0>{});
    if (sl + 1 < ns) slab(sl + 1, std::integral_constant<int, 1>{});
  }
  // register e of lane (i, g) of sub-tile (s, s2) = C[own column 16 s + 4g + e]
  // [partner column 16 s2 + i]; straight to the slabs
  const int bx = wave >> 1;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int yt = (pk >> (3 * j)) & 7, by = yt >> 1;
    const int code = gram_product(bx, by), pr = code & 7;
    const size_t sidx = pr < 2 ? (size_t)(2 * q + pr) * nchunk + chunk
                               : (size_t)P * nchunk + ((size_t)q * 4 + (pr - 2)) * nchunk + chunk;
    float* out = slabs + sidx * (W * W);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const f32x4 v = acc[j][s][s2] + lo[j][s][s2];
        const int xr = 32 * (wave & 1) + 16 * s + 4 * g, yc = 32 * (yt & 1) + 16 * s2 + i16;
        if (code & 8) {  // slab rows are the partner's block
          *reinterpret_cast<f32x4*>(out + yc * W + xr) = v;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) out[(xr + e) * W + yc] = v[e];
        }
      }
  }
}

}  // namespace svdj
