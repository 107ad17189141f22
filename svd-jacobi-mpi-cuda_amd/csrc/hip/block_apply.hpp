// Apply stage of the block Jacobi step (block.hip), single steps: for the
// P block pairs (bi, bj) of a step, X = [A_bi A_bj] (m x 2W),
//     apply : X <- X Q and [V_bi V_bj] <- [..] Q in place, MFMA, computed
//             transposed (Out^T = Q^T X^T) so loads AND stores are
//             128-byte coalesced column segments.
// On f32 / f64 MFMA (apply_kernel) or, fp32 data, on bf16 MFMA from split
// operands (apply_split_kernel; the split helpers also serve block_quad.hpp).
#pragma once
#include "block_evd.hpp"  // half_swap
#include "common.hpp"

#include <type_traits>

namespace svdj {

constexpr int kApplyThreads = 256;

// ------------------------------------------------------------------ apply
// Q fragments are read kQPD k-steps ahead of their MFMA (row-layout Q).
constexpr int kQPD = 8;
template <typename T, int W>
__host__ __device__ constexpr int apply_threads() { return kApplyThreads; }
template <typename T, int W>
__global__ __launch_bounds__((apply_threads<T, W>())) void apply_kernel(
    T* __restrict__ A, int lda, int a_chunks, int rows_a, int m_pad, T* __restrict__ V,
    int ldv, int rows_v, int n_v, const int32_t* __restrict__ pairs, const T* __restrict__ Qall,
    const int32_t* __restrict__ skip) {
  using M = Mfma<T>;
  constexpr int TL = M::TILE;
  constexpr int KG = M::KG;
  constexpr int N = 2 * W;
  constexpr int NK = N / KG;   // k values per lane
  constexpr int NCT = N / TL;  // output column tiles
  constexpr int LDQ = N + (sizeof(T) == 8 ? 16 : 0);
  constexpr int NTH = apply_threads<T, W>();
  constexpr int WAVES = NTH / SVDJ_WAVE;
  __shared__ alignas(16) T Qs[N * LDQ];

  const int pair = blockIdx.x;
  if (skip[pair]) return;
  const int bi = pairs[2 * pair], bj = pairs[2 * pair + 1];
  int chunk = blockIdx.y;
  T* base;
  int ld, r_begin, r_end;
  if (chunk < a_chunks) {
    base = A;
    ld = lda;
    r_begin = chunk * rows_a;
    r_end = min(m_pad, r_begin + rows_a);
  } else {
    chunk -= a_chunks;
    base = V;
    ld = ldv;
    r_begin = chunk * rows_v;
    r_end = min(n_v, r_begin + rows_v);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = M::lane_col(lane), kg = M::lane_kg(lane);
  // Column k of X = [A_bi A_bj] is base + col(k)*ld.  The lane-dependent
  // part of every address (k group, row lane, acc row group) is folded into
  // one 64-bit lane offset; the per-k / per-tile part is wave-uniform, so the
  // address arithmetic stays in SGPRs.
  T* const xi = base + (size_t)bi * W * ld;
  T* const xj = base + (size_t)bj * W * ld;
  const uint32_t ld_off = (uint32_t)(kg * ld + lc);
  const uint32_t st_off = (uint32_t)(M::acc_row_lane(lane) * ld + lc);
  // Q fragments are loop-invariant: small Q (<= 64 VGPRs of fragments) is
  // left to the compiler to hoist into registers; larger Q is re-read from
  // LDS per row tile (the empty asm with a memory clobber blocks the hoist).
  constexpr bool kHoistQ = (NK * NCT * (int)sizeof(T)) / 4 <= 64;
  auto load_tile = [&](T (&x)[NK], int r) {
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) {
      const int k0 = kk * KG;
      const T* src = (k0 < W ? xi + (size_t)k0 * ld : xj + (size_t)(k0 - W) * ld);
      x[kk] = src[ld_off + (uint32_t)r];
    }
  };
  int r0 = r_begin + wave * TL;
  T xv[NK];
  const T* Qg = Qall + (size_t)pair * N * N;
  // fp64: Q in A-operand fragment order -- for (column tile, group of VEC
  // k-steps, lane) the VEC operands are contiguous, one 16-byte LDS read per
  // VEC MFMAs (fp64 W=64 apply 912 -> 845 us; fp32 W=64 319 -> 338 us, so
  // fp32 keeps the row layout with an element-wise fill -- 16-byte and
  // LDS-DMA fills measured slower or equal, round 2)
  constexpr bool kQFrag = sizeof(T) == 8;
  constexpr int VEC = 16 / (int)sizeof(T);
  using QV = __attribute__((ext_vector_type(VEC))) T;
  const QV* Qgv = reinterpret_cast<const QV*>(Qg);
  if constexpr (kQFrag) {
    for (int iv = threadIdx.x; iv < N * N / VEC; iv += NTH) {
      const QV q = Qgv[iv];
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const int i = iv * VEC + u;
        const int k = i / N, c = i % N;
        const int kk = k / KG, kgi = k % KG, ct = c / TL, lci = c % TL;
        Qs[((ct * (NK / VEC) + kk / VEC) * 64 + kgi * TL + lci) * VEC + kk % VEC] = q[u];
      }
    }
  } else {
    for (int i = threadIdx.x; i < N * N; i += NTH) Qs[(i / N) * LDQ + (i % N)] = Qg[i];
  }
  __syncthreads();
  if (r0 >= r_end) return;
  load_tile(xv, r0);
  while (true) {
    const int rn = r0 + WAVES * TL;
    const bool more = rn < r_end;
    T xn[NK];
    if (more) load_tile(xn, rn);  // next tile in flight during this tile's MFMAs
    if constexpr (!kHoistQ) asm volatile("" ::: "memory");
    constexpr int kCtUnroll = kHoistQ ? NCT : 1;
#pragma unroll kCtUnroll
    for (int ct = 0; ct < NCT; ++ct) {
      typename M::acc_t acc = M::zero();
      if constexpr (kQFrag) {
        using V4 = __attribute__((ext_vector_type(VEC))) T;
        const V4* qv = reinterpret_cast<const V4*>(Qs) + (size_t)ct * (NK / VEC) * 64 + lane;
        V4 cur = qv[0];
#pragma unroll
        for (int g = 0; g < NK / VEC; ++g) {
          V4 nxt = cur;
          if (g + 1 < NK / VEC) nxt = qv[(g + 1) * 64];
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc = M::mfma(cur[e], xv[g * VEC + e], acc);
          cur = nxt;
        }
      } else {
        // Q fragments are read kQPD k-steps ahead of their MFMA (sched_barrier
        // keeps the order; just in time, each ds_read's latency sat between
        // two dependent MFMAs).  Two interleaved accumulation chains per wave
        // were measured slower (1269 vs 1145 us, W=64).
        constexpr int PD = kQPD < NK ? kQPD : NK;
        T qa[PD];
#pragma unroll
        for (int i = 0; i < PD; ++i) qa[i] = Qs[(i * KG + kg) * LDQ + ct * TL + lc];
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) {
          const T a = qa[kk % PD];
          if (kk + PD < NK) qa[kk % PD] = Qs[((kk + PD) * KG + kg) * LDQ + ct * TL + lc];
          acc = M::mfma(a, xv[kk], acc);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      const int c0 = ct * TL;
      T* dst = (c0 < W ? xi + (size_t)c0 * ld : xj + (size_t)(c0 - W) * ld);
#pragma unroll
      for (int e = 0; e < M::NACC; ++e)
        dst[(size_t)M::acc_row_uni(e) * ld + (st_off + (uint32_t)r0)] = acc[e];
    }
    if (!more) break;
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) xv[kk] = xn[kk];
    r0 = rn;
  }
}

// A wave-uniform pointer moved to SGPRs (v_readfirstlane), so an access
// p[lane offset] can use the scalar-base + 32-bit VGPR offset address form.
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<T*>(((uint64_t)hi << 32) | lo);
}

// Element i of a base pointer with a 32-bit byte offset (the caller
// guarantees i * sizeof(T) < 2^32): for a wave-uniform base the address is
// SGPR base + 32-bit VGPR offset instead of a 64-bit VGPR address.
template <typename T>
__device__ __forceinline__ T& at_u32(T* base, uint32_t i) {
  using B = typename std::conditional<std::is_const<T>::value, const char, char>::type;
  return *reinterpret_cast<T*>(reinterpret_cast<B*>(base) + i * (uint32_t)sizeof(T));
}

// -------------------------------------------------- apply on bf16 matrix cores
// fp32 data, bf16 MFMA (v_mfma_f32_32x32x16_bf16, 16x the f32 MFMA rate):
// every operand is split into NP round-to-nearest bf16 parts,
//   x = x0 + x1 + x2,  |x - x0| <= 2^-9|x|, |x - x0 - x1| <= 2^-18|x|, ...
// and the products of total order < NP are accumulated in fp32 (bf16 x bf16
// products are exact):  NP = 3 -> 6 MFMAs (00 01 10 02 11 20), dropped terms
// are O(2^-26)|x||q|, i.e. fp32 rounding level;  NP = 2 -> 3 MFMAs, O(2^-18)
// (the "bf16x3" fast mode).  The 2W x 2W Q is split once per workgroup into
// LDS, already in A-operand fragment order (one ds_read_b128 per part);
// the X tile is split in registers right after its loads land.
// Same transposed formulation as apply_kernel: Out^T = Q^T X^T, lane = row.

template <int NP>
__device__ __forceinline__ void split_bf16(float x, __bf16 (&p)[NP]) {
  float r = x;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    p[i] = (__bf16)r;  // round to nearest even
    r -= (float)p[i];
  }
}

// Eight values at once, two per instruction: v_cvt_pk_bf16_f32 rounds a pair,
// the pair goes back to fp32 with a shift and a mask, and one v_pk_add_f32
// takes both remainders -- 4.5 VALU instructions per value and 3 parts
// instead of 7.5 for split_bf16 one value at a time (the compiler converts
// each scalar alone), bitwise the same parts.
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x2 = __attribute__((ext_vector_type(2))) float;
template <int NP>
__device__ __forceinline__ void split_bf16x8(const float (&v)[8], bf16x8 (&parts)[NP]) {
  f32x2 r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = f32x2{v[2 * j], v[2 * j + 1]};
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    bf16x2 p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      p[j] = __builtin_convertvector(r[j], bf16x2);
      if (i + 1 < NP) r[j] -= __builtin_convertvector(p[j], f32x2);
    }
    parts[i] = __builtin_shufflevector(__builtin_shufflevector(p[0], p[1], 0, 1, 2, 3),
                                       __builtin_shufflevector(p[2], p[3], 0, 1, 2, 3), 0, 1, 2, 3,
                                       4, 5, 6, 7);
  }
}

// Products of total order >= LO (small terms first).
template <int NP, int LO>
__device__ __forceinline__ f32x16 mfma_split(const bf16x8 (&q)[NP], const bf16x8 (&x)[NP],
                                             f32x16 acc) {
#pragma unroll
  for (int ord = NP - 1; ord >= LO; --ord)
#pragma unroll
    for (int a = 0; a <= ord; ++a)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q[a], x[ord - a], acc, 0, 0, 0);
  return acc;
}

// Waves own OUTPUT COLUMN tiles, not rows: wave w computes the 32 output
// columns ct = w % NCT of the row tile (row group w / NCT; W = 64: all four
// waves on one 32-row tile, W = 32: two 32-row tiles), so its split Q - I
// fragments (NKB x NP bf16x8, 96 VGPRs for W = 64) stay in registers for
// the whole workgroup.  The X tile is loaded once: wave w loads and splits
// the k columns of its own output tile (k blocks 2ct, 2ct+1) into an LDS
// image in B-fragment order (double-buffered, one barrier per tile), and
// keeps those raw fp32 values for the epilogue Y = X + X (Q - I), where a
// v_permlane32_swap moves them from the B-operand lanes to the accumulator
// lanes.  No operand is re-read from global memory.
//
// Delta form (Q - I): the identity part is never rounded inside the
// MFMA.  The bf16 MFMA's internal accumulation is not IEEE round-to-nearest,
// and with X Q directly a dominant diagonal term biased every sum (column
// norms drifted 780 eps in 400 near-identity applies, round 1); with the
// identity added back in fp32 the drift is 0.14-0.17 eps against 3 eps for
// the f32 MFMA (tools/probe_apply.py, profiles/r3_s3/bf16x6).
template <int W, int NP>
__global__ __launch_bounds__(kApplyThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void apply_split_kernel(
    float* __restrict__ A, int lda, int a_chunks, int rows_a, int m_pad, float* __restrict__ V,
    int ldv, int rows_v, int n_v, const int32_t* __restrict__ pairs,
    const float* __restrict__ Qall, const int32_t* __restrict__ skip, int vfirst) {
  constexpr int N = 2 * W;
  constexpr int NCT = N / 32;                   // output column tiles
  constexpr int NKB = N / 16;                   // 16-deep k blocks
  constexpr int WAVES = kApplyThreads / SVDJ_WAVE;
  constexpr int RG = WAVES / NCT;               // 32-row groups per tile
  constexpr int TR = 32 * RG;                   // rows per tile
  static_assert(NCT * RG == WAVES && NKB == 2 * NCT, "wave <-> (column tile, row group)");
  static_assert(W % 16 == 0, "k blocks must not straddle the two column blocks");
  __shared__ bf16x8 Xf[2][RG][NKB][NP][SVDJ_WAVE];

  const int pair = blockIdx.x;
  if (skip[pair]) return;
  const int bi = pairs[2 * pair], bj = pairs[2 * pair + 1];
  // vfirst: V's row chunks dispatched before A's, so A's rows are the most
  // recently written when the next step's Gram reads them
  const int vch = gridDim.y - a_chunks;
  int chunk = vfirst ? (blockIdx.y < (unsigned)vch ? a_chunks + (int)blockIdx.y : (int)blockIdx.y - vch)
                     : (int)blockIdx.y;
  float* base;
  int ld, r_begin, r_end;
  if (chunk < a_chunks) {
    base = A;
    ld = lda;
    r_begin = chunk * rows_a;
    r_end = min(m_pad, r_begin + rows_a);
  } else {
    chunk -= a_chunks;
    base = V;
    ld = ldv;
    r_begin = chunk * rows_v;
    r_end = min(n_v, r_begin + rows_v);
  }
  if (r_begin >= r_end) return;
  // wave index through readfirstlane: everything derived from it (own) is
  // known uniform and stays in SGPRs
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 31, h = lane >> 5;
  const int ct = wave % NCT, rg = wave / NCT;
  float* const xi = base + (size_t)bi * W * ld;
  float* const xj = base + (size_t)bj * W * ld;
  // the wave's own 32 columns (k blocks 2ct, 2ct+1 = output tile ct)
  float* const own = ct * 32 < W ? xi + (size_t)(ct * 32) * ld : xj + (size_t)(ct * 32 - W) * ld;

  // Q - I fragments of column tile ct: (kb, lane) = Q[kb*16 + 8h + e][ct*32 + c] - delta
  bf16x8 qf[NKB][NP];
  {
    const float* Qg = Qall + (size_t)pair * N * N + ct * 32 + c;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = kb * 16 + 8 * h + e;
        __bf16 p[NP];
        split_bf16<NP>(Qg[(size_t)k * N] - (k == ct * 32 + c ? 1.0f : 0.0f), p);
#pragma unroll
        for (int i = 0; i < NP; ++i) qf[kb][i][e] = p[i];
      }
  }
  // raw X of this wave's k blocks for rows r .. r+31: x[kbl][e] = X[r + c][ct*32 + 16 kbl + 8h + e].
  // Column bases are wave-uniform (SGPRs, readfirstlane) with a 32-bit lane
  // offset, so the loads use the scalar-base address form instead of one
  // 64-bit VGPR address per column (32 VGPRs the operand prefetch needs).
  const uint32_t lane_off = (uint32_t)(8 * h * ld + c);
  auto load = [&](float (&x)[2][8], int r) {
#pragma unroll
    for (int kbl = 0; kbl < 2; ++kbl)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        x[kbl][e] = at_u32(own + (size_t)(16 * kbl + e) * ld, lane_off + (uint32_t)r);
  };
  const uint32_t st_off = (uint32_t)(4 * h * ld + c);
  // Loads run two tiles ahead: tile t's raw values are in one register set
  // while tile t+1's are in flight in the other (the loop is unrolled by two
  // so both sets are static); tile t+2 is issued into the first set as soon
  // as tile t's values are in LDS and in the epilogue registers.  One tile of
  // look-ahead left ~16 KB in flight per workgroup, short of what the HBM
  // latency under load needs.
  auto tile = [&](float (&xr)[2][8], int t) -> bool {
    const int rt = r_begin + t * TR;
    if (rt >= r_end) return false;  // uniform over the workgroup
    const int buf = t & 1;
    const int r0 = rt + rg * 32;      // this wave's rows
    const bool mine = r0 < r_end;
    // split this tile's own k blocks into the shared B-fragment image
    if (mine) {
#pragma unroll
      for (int kbl = 0; kbl < 2; ++kbl) {
        bf16x8 parts[NP];
        split_bf16x8<NP>(xr[kbl], parts);
#pragma unroll
        for (int i = 0; i < NP; ++i) Xf[buf][rg][2 * ct + kbl][i][lane] = parts[i];
      }
    }
    // epilogue operand: own raw values moved to accumulator lanes.  Output
    // register g*4+i of lane (c, h) is column 8g + 4h + i of the tile; lane
    // half h holds columns 16 kbl + 8h + e.
    float xo[16];
#pragma unroll
    for (int kbl = 0; kbl < 2; ++kbl)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float keep = h ? xr[kbl][4 + i] : xr[kbl][i];
        const float give = h ? xr[kbl][i] : xr[kbl][4 + i];
        const float got = __int_as_float(half_swap(__float_as_int(give)));
        xo[(2 * kbl) * 4 + i] = h ? got : keep;
        xo[(2 * kbl + 1) * 4 + i] = h ? keep : got;
      }
    if (r0 + 2 * TR < r_end) load(xr, r0 + 2 * TR);
    __syncthreads();
    if (mine) {
      f32x16 acc = Mfma<float>::zero(), lo = Mfma<float>::zero();
      // B operands of k block kb + 1 are read while kb's MFMAs run
      bf16x8 xs[NP], xn[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) xs[i] = Xf[buf][rg][0][i][lane];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        if (kb + 1 < NKB) {
#pragma unroll
          for (int i = 0; i < NP; ++i) xn[i] = Xf[buf][rg][kb + 1][i][lane];
        }
        // the high-order product in its own accumulator, the small terms in
        // a second one
        lo = mfma_split<NP, 1>(qf[kb], xs, lo);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[kb][0], xs[0], acc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NP; ++i) xs[i] = xn[i];
      }
      acc += lo;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        at_u32(own + (size_t)Mfma<float>::acc_row_uni(e) * ld, st_off + (uint32_t)r0) = xo[e] + acc[e];
    }
    return true;
  };
  float xa[2][8], xb[2][8];
  const int r0 = r_begin + rg * 32;
  if (r0 < r_end) load(xa, r0);
  if (r0 + TR < r_end) load(xb, r0 + TR);
  for (int t = 0;; t += 2) {
    if (!tile(xa, t)) break;
    if (!tile(xb, t + 1)) break;
  }
}

}  // namespace svdj
