// llt_tile.h -- the 64x64 fp64 tile primitives of the reduced-system Cholesky,
// shared by its two executors (llt_levels.hip, llt_dag.hip), the selected
// inverse (selinv.hip) and the micro-benchmarks under tools/: LDS pitches,
// tile loads and stores, the 16x16 diagonal block (diag16), the blocked 64x64
// factorization, triangular solve and inverse, and the 4-wave MFMA GEMM.
//
// Everything sits in an anonymous namespace on purpose: every translation unit
// gets its own internal copy (as when this was one .hip file), and a kernel
// keeps the mangled name it had there.  blocked_potrf64, blocked_trsm64 and
// blocked_trinv64 are forceinline: left to the inliner, k_panel's machine code
// depended on which other kernels of its translation unit called them too
// (profiles/llt_split/README.md).
#pragma once

#include "llt_plan.h"
#include "lm_problem.h"   // kTile

#include <utility>

namespace arslam {

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));
typedef double dbl2 __attribute__((ext_vector_type(2)));

constexpr int T64 = kTile;

#ifdef ARSLAM_STAMPS
__device__ unsigned long long g_stamps[64];
#define STAMP(id)                                                                       \
  do {                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                  \
    unsigned long long _t;                                                              \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");        \
    if (blockIdx.x == 0 && threadIdx.x == 0) g_stamps[id] = _t;                         \
    __builtin_amdgcn_sched_barrier(0);                                                  \
  } while (0)
#else
#define STAMP(id) do {} while (0)
#endif

constexpr int LM = 66;   // LDS row pitch of k_update's MFMA operand tiles (conflict-free ds_read_b64)
constexpr int LQ = 66;   // LDS pitch of the blocked panel kernel (16-lane row access and MFMA
                         // fragment reads both conflict-free)
constexpr int LI = 18;   // LDS pitch of the 16x16 inverse diagonal blocks (conflict-free fragments)
constexpr int kLtdSize = 4 * 16 * LI;   // a tile column's four 16x16 block inverses: 1152 doubles

// Compact tile storage: tile (i,j) of the factor is a contiguous 64x64
// row-major block at S + tid[i*T + j] * 4096 (tid = -1: structurally zero).
__device__ __forceinline__ double *tile_ptr(double *S, const int *tid, int T, int i, int j) {
  return S + (long)tid[(long)i * T + j] * (T64 * T64);
}
__device__ __forceinline__ const double *tile_ptr(const double *S, const int *tid, int T, int i, int j) {
  return S + (long)tid[(long)i * T + j] * (T64 * T64);
}

// 256-thread load of a 64x64 tile into LDS (pitch LQ), all loads in flight.
__device__ __forceinline__ void load_tile_wg(const double *__restrict__ g, long lda, double *lds,
                                             int tid) {
  dbl2 v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    v[q] = *reinterpret_cast<const dbl2 *>(g + (long)r * lda + c2);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    *reinterpret_cast<dbl2 *>(lds + r * LQ + c2) = v[q];
  }
}

// 256-thread store of the lower triangle (zeros above) of an LDS tile.
__device__ __forceinline__ void store_tile_wg(double *__restrict__ g, long lda, const double *lds,
                                              int tid, bool lower_only) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    dbl2 v = *reinterpret_cast<const dbl2 *>(lds + r * LQ + c2);
    if (lower_only) {
      if (c2 > r) v.x = 0.0;
      if (c2 + 1 > r) v.y = 0.0;
    }
    *reinterpret_cast<dbl2 *>(g + (long)r * lda + c2) = v;
  }
}

// v of lane l of this lane's 16-lane row: one v_mov_b64_dpp row_newbcast:l.
// l must fold to a constant (unrolled loops; the switch then disappears), and
// the source lane must be active: call it outside divergent conditions.
__device__ __forceinline__ double bcast16(double v, int l) {
  switch (l) {
    case 0: return __builtin_amdgcn_mov_dpp(v, 0x150, 0xf, 0xf, false);
    case 1: return __builtin_amdgcn_mov_dpp(v, 0x151, 0xf, 0xf, false);
    case 2: return __builtin_amdgcn_mov_dpp(v, 0x152, 0xf, 0xf, false);
    case 3: return __builtin_amdgcn_mov_dpp(v, 0x153, 0xf, 0xf, false);
    case 4: return __builtin_amdgcn_mov_dpp(v, 0x154, 0xf, 0xf, false);
    case 5: return __builtin_amdgcn_mov_dpp(v, 0x155, 0xf, 0xf, false);
    case 6: return __builtin_amdgcn_mov_dpp(v, 0x156, 0xf, 0xf, false);
    case 7: return __builtin_amdgcn_mov_dpp(v, 0x157, 0xf, 0xf, false);
    case 8: return __builtin_amdgcn_mov_dpp(v, 0x158, 0xf, 0xf, false);
    case 9: return __builtin_amdgcn_mov_dpp(v, 0x159, 0xf, 0xf, false);
    case 10: return __builtin_amdgcn_mov_dpp(v, 0x15a, 0xf, 0xf, false);
    case 11: return __builtin_amdgcn_mov_dpp(v, 0x15b, 0xf, 0xf, false);
    case 12: return __builtin_amdgcn_mov_dpp(v, 0x15c, 0xf, 0xf, false);
    case 13: return __builtin_amdgcn_mov_dpp(v, 0x15d, 0xf, 0xf, false);
    case 14: return __builtin_amdgcn_mov_dpp(v, 0x15e, 0xf, 0xf, false);
    case 15: return __builtin_amdgcn_mov_dpp(v, 0x15f, 0xf, 0xf, false);
    default: return v;
  }
}

// One wave: C(16x16) -= A(16 x K) B(16 x K)^T, operands in LDS (pitch LQ;
// C never overlaps A or B).  C's four entries per lane are read before the
// MFMA chain: read after it, hipcc issued each read-subtract-write as its own
// LDS round trip (four in a row, ~300 cycles on the POTRF's chain per call).
__device__ __forceinline__ void wave_gemm16_sub(double *C, const double *A, const double *B, int K,
                                                int lane) {
  const int li = lane & 15, lk = lane >> 4;
  double c[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) c[reg] = C[(lk + 4 * reg) * LQ + li];
  dbl4 acc = {0, 0, 0, 0};
  for (int k4 = 0; k4 < K; k4 += 4) {
    const double a = A[li * LQ + k4 + lk];
    const double b = B[li * LQ + k4 + lk];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) C[(lk + 4 * reg) * LQ + li] = c[reg] - acc[reg];
}


// One wave: C(16x16) <- C Linv^T in place (the 16-column triangular solve
// X L^T = C as an MFMA product with the explicit inverse of the 16x16 block).
__device__ __forceinline__ void wave_apply_inv16(double *C, const double *Linv, int lane) {
  const int li = lane & 15, lk = lane >> 4;
  double a[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = C[li * LQ + 4 * q + lk];
  __builtin_amdgcn_wave_barrier();
  dbl4 acc = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], Linv[li * LI + 4 * q + lk], acc, 0, 0, 0);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) C[(lk + 4 * reg) * LQ + li] = acc[reg];
}

// One elimination step of diag16 under an explicit exec mask (constant per
// pivot, so no per-lane selects): in the rows below the pivot,
// x_q += nf * xj_q and R += nf * rj; then, in the pivot column's group,
// register jq becomes nf.  The masks are 32-bit immediates per exec half
// (both halves of `below` are equal), so no SGPR pair holds a 64-bit mask
// constant across the unrolled pivots (those used to be spilled to VGPR lanes
// and reloaded with v_readlane inside the chain).  The caller's exec is
// restored at the end, and the trailing s_nop covers the wait states hipcc
// does not insert after an asm statement (exec write -> DPP, and the outputs
// -> the next pivot's DPP).
template <int j>
__device__ __forceinline__ void elim_step(double &x0, double &x1, double &x2, double &x3, double &R, double nf,
                                          double y0, double y1, double y2, double y3, double rj) {
  constexpr unsigned m = (0xffffu << (j + 1)) & 0xffffu;   // rows i > j of one 16-lane group
  constexpr unsigned BL = m | (m << 16);                    // `below`, per exec half
  constexpr int g = j >> 2;                                 // the group holding column j
  constexpr unsigned CL = g == 0 ? m : g == 1 ? (m << 16) : 0u;
  constexpr unsigned CH = g == 2 ? m : g == 3 ? (m << 16) : 0u;
  unsigned sl, sh;
#define ARSLAM_ELIM_ASM(XS)                                                                   \
  asm volatile("s_mov_b32 %[sl], exec_lo\n\t"                                                 \
               "s_mov_b32 %[sh], exec_hi\n\t"                                                 \
               "s_and_b32 exec_lo, %[sl], %[bl]\n\t"                                          \
               "s_and_b32 exec_hi, %[sh], %[bl]\n\t"                                          \
               "v_fma_f64 %[x0], %[nf], %[y0], %[x0]\n\t"                                     \
               "v_fma_f64 %[x1], %[nf], %[y1], %[x1]\n\t"                                     \
               "v_fma_f64 %[x2], %[nf], %[y2], %[x2]\n\t"                                     \
               "v_fma_f64 %[x3], %[nf], %[y3], %[x3]\n\t"                                     \
               "v_fma_f64 %[R], %[nf], %[rj], %[R]\n\t"                                       \
               "s_and_b32 exec_lo, %[sl], %[cl]\n\t"                                          \
               "s_and_b32 exec_hi, %[sh], %[ch]\n\t"                                          \
               "v_mov_b64 %[" XS "], %[nf]\n\t"                                               \
               "s_mov_b32 exec_lo, %[sl]\n\t"                                                 \
               "s_mov_b32 exec_hi, %[sh]\n\t"                                                 \
               "s_nop 4"   /* exec write -> DPP: 5 states; VGPR write -> DPP read: 2 */        \
               : [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2), [x3] "+v"(x3), [R] "+v"(R),      \
                 [sl] "=&s"(sl), [sh] "=&s"(sh)                                                \
               : [nf] "v"(nf), [y0] "v"(y0), [y1] "v"(y1), [y2] "v"(y2), [y3] "v"(y3),          \
                 [rj] "v"(rj), [bl] "i"(BL), [cl] "i"(CL), [ch] "i"(CH))
  switch (j & 3) {
    case 0: ARSLAM_ELIM_ASM("x0"); break;
    case 1: ARSLAM_ELIM_ASM("x1"); break;
    case 2: ARSLAM_ELIM_ASM("x2"); break;
    default: ARSLAM_ELIM_ASM("x3"); break;
  }
#undef ARSLAM_ELIM_ASM
}

// Pivot J of diag16 (a template, so every broadcast lane and exec mask is a
// compile-time constant however large the unrolled loop gets).
template <int j>
__device__ __forceinline__ void diag16_pivot(double (&x)[4], double &R, double &R2, double *colx, int lane) {
  const int i = lane & 15;
  const double ajj = bcast16(R, j);
  const double r0 = __builtin_amdgcn_rcp(ajj);
  const double e = __builtin_fma(-ajj, r0, 1.0);   // r0 (1 + e + e^2) = (1 - e^3) / ajj
  const double nf0 = -R * r0;
  const double pe = __builtin_fma(e, e, e);
  const double nf = __builtin_fma(nf0, pe, nf0);    // -f_ij (garbage in rows i <= j: masked below)
  double xj[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) xj[q] = bcast16(x[q], j);
  const double rj = j + 1 < 16 ? bcast16(R2, j) : 0.0;
  R = R2;
  // rows i > j only (exec = the lanes 16 g + i with i > j, a constant per
  // pivot); then column j of those rows (group j / 4) becomes -f_ij
  elim_step<j>(x[0], x[1], x[2], x[3], R, nf, xj[0], xj[1], xj[2], xj[3], rj);
  if (j + 2 < 16) {   // column j+2 after this pivot, a pivot before it is needed
    colx[lane] = x[(j + 2) & 3];
    R2 = colx[16 * ((j + 2) >> 2) + i];
  }
}

template <int... J>
__device__ __forceinline__ void diag16_pivots(double (&x)[4], double &R, double &R2, double *colx, int lane,
                                              std::integer_sequence<int, J...>) {
  (diag16_pivot<J>(x, R, R2, colx, lane), ...);
}

// 16x16 diagonal block (rows/cols b0..b0+15 of D, lower triangle) on one
// wave: L into D (zeros above the diagonal), L^{-1} into Li (pitch LI),
// 1/L_ii into inv.  Lane 16 g + i owns row i, columns 4g..4g+3.  One
// Gaussian elimination pass over A, in place: at pivot j the register of
// column j in the rows below becomes the multiplier -f_ij, so row i ends as
// U = Dg Lu^T (columns >= i) and Lu^{-1} (columns < i), with Lu unit lower
// and Dg the pivots; then L^T = Dg^{-1/2} U and L^{-1} = Dg^{-1/2} Lu^{-1}.
// Each pivot needs column j in every row; it is kept replicated one pivot
// ahead (R: column j, R2: column j+1), and column j+2 is fetched through the
// 64-double LDS scratch colx after pivot j's update, a pivot before it is
// needed.  Per pivot: DPP broadcast -> v_rcp_f64 -> two-term Newton
// correction -> multiplier -> update; about 20 VALU instructions, so the
// block is bound by one wave's issue rate (tools/lat_bench.hip).
__device__ __forceinline__ void diag16(double *D, int b0, double *inv, double *Li, int *bad, int lane,
                                       double *colx) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int g = lane >> 4, i = lane & 15;
  double x[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {   // the lower triangle is the valid half: mirror it
    const int c = 4 * g + q;
    x[q] = c <= i ? D[(b0 + i) * LQ + b0 + c] : D[(b0 + c) * LQ + b0 + i];
  }
  // replicated columns 0 and 1 (lower triangle mirrored)
  double R = D[(b0 + i) * LQ + b0];
  double R2 = i >= 1 ? D[(b0 + i) * LQ + b0 + 1] : D[(b0 + 1) * LQ + b0];
  diag16_pivots(x, R, R2, colx, lane, std::make_integer_sequence<int, 16>{});
  // pivot of row i: the diagonal entry of U, held by group i / 4
  __builtin_amdgcn_wave_barrier();
  if (g == (i >> 2)) colx[i] = (i & 3) == 0 ? x[0] : (i & 3) == 1 ? x[1] : (i & 3) == 2 ? x[2] : x[3];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const double piv = colx[i];
  if (!(piv > 0.0)) *bad = 1;
  const double d = sqrt(piv), rd = 1.0 / d;
  // lane (g, i), column c = 4g+q:  L_{c,i} = U_i[c] / d_i (c > i),
  // (L^{-1})_{i,c} = Lu^{-1}_i[c] / d_i (c < i)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = 4 * g + q;
    D[(b0 + c) * LQ + b0 + i] = c > i ? x[q] * rd : (c == i ? d : 0.0);
    Li[i * LI + c] = c < i ? x[q] * rd : (c == i ? rd : 0.0);
  }
  if (g == 0) inv[b0 + i] = rd;
}

// In-LDS blocked Cholesky of the 64x64 tile D (256 threads), right-looking
// over 16-column panels with a one-panel lookahead: wave 0 updates the next
// diagonal block first and factors it (diag16) while waves 1-3 apply the
// rest of the trailing update, so the critical chain is the four diag16
// calls plus one 16-row solve and one 16x16 update per panel.
// Returns false (uniformly) if a pivot is not positive; inv[c] = 1 / L_cc.
// idle(p, w, lane) runs on waves 1-3 beside wave 0's diagonal block p (after
// their share of the trailing update): the persistent executor fetches its
// fused TRSM's tile there.
// F (with fold / non-null): a 64x64 tile in LDS (pitch LQ) whose product F F^T is first
// subtracted from D -- the last update of the diagonal tile, folded into the
// factorization: wave 0 folds block (0,0) and goes straight on to its
// diag16 while waves 1-3 fold the other nine lower blocks beside it (the
// same MFMA products in the same order as a separate fold: bit-identical).
template <class Idle>
__device__ bool blocked_potrf64_idle(double *D, double *inv, double *LTd, int *bad, int tid, double *colx,
                                     Idle &&idle, const double *F = nullptr) {
  const int w = tid >> 6, lane = tid & 63;
  if (tid == 0) *bad = 0;
  __syncthreads();
  for (int p = 0; p < 4; ++p) {
    const int b0 = 16 * p;
    STAMP(10 + 4 * p);
    if (w == 0) {
      if (p == 0 && F) wave_gemm16_sub(D, F, F, 64, lane);
      if (p > 0) wave_gemm16_sub(D + b0 * LQ + b0, D + b0 * LQ + b0 - 16, D + b0 * LQ + b0 - 16, 16, lane);
      diag16(D, b0, inv, LTd + p * 16 * LI, bad, lane, colx);
    } else if (p == 0) {
      if (F) {
        // lower blocks 1..9 in row order (I, C), I >= C: (1,0) (1,1) (2,0) (2,1) (2,2) (3,0) ...
        for (int t = w; t < 10; t += 3) {
          int I = 0;
          while ((I + 1) * (I + 2) / 2 <= t) ++I;
          const int C = t - I * (I + 1) / 2;
          wave_gemm16_sub(D + 16 * I * LQ + 16 * C, F + 16 * I * LQ, F + 16 * C * LQ, 64, lane);
        }
      }
      idle(0, w, lane);
    } else {
      // panel p-1's update of blocks (I, C), I >= C >= p, except (p, p)
      const int m = 4 - p, ntl = m * (m + 1) / 2;
      for (int t = w; t < ntl; t += 3) {
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        const int C = t - I * (I + 1) / 2;
        const int bi = 16 * (p + I), bc = 16 * (p + C);
        wave_gemm16_sub(D + bi * LQ + bc, D + bi * LQ + b0 - 16, D + bc * LQ + b0 - 16, 16, lane);
      }
      idle(p, w, lane);
    }
    __syncthreads();
    STAMP(11 + 4 * p);
    if (p < 3) {
      // rows below the diagonal block: X L_pp^T = A_panel  ->  X = A_panel L_pp^{-T}
      if (w < 3 - p) wave_apply_inv16(D + (b0 + 16 + 16 * w) * LQ + b0, LTd + p * 16 * LI, lane);
      __syncthreads();
    }
    STAMP(12 + 4 * p);
    STAMP(13 + 4 * p);
  }
  return *bad == 0;
}

// LDS flags of the asynchronous panel pipeline below (one workgroup).  The
// volatile accesses go through LDS-typed pointers: a volatile access through a
// generic pointer stays a flat access (the address space is not inferred),
// and hipcc mis-selects the aperture compare of some of those.
typedef __attribute__((address_space(3))) volatile int lds_vint;
__device__ __forceinline__ lds_vint *as_lds(const int *f) { return (lds_vint *)(f); }
__device__ __forceinline__ void lds_set(int *f, int v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  *as_lds(f) = v;
}
__device__ __forceinline__ void lds_add(int *f, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (lane == 0) __hip_atomic_fetch_add(f, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int lds_get(const int *f) { return *as_lds(f); }
__device__ __forceinline__ void lds_wait(const int *f, int v) {
  while (*as_lds(f) < v) __builtin_amdgcn_s_sleep(0);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The same factorization (same products in the same order: bit-identical) as
// blocked_potrf64_idle, without workgroup barriers on wave 0's chain.  Wave 0
// runs diag16(p) -> the next block's apply (p+1, p) -> the lookahead update of
// (p+1, p+1) -> diag16(p+1) ...; waves 1-3 apply the blocks further down and
// do the trailing updates of each panel (and the optional fold F F^T) beside
// it, synchronised through the LDS counters fl[kPf*] (PotrfFlag below).
// idle(p, w, lane) runs on waves 1-3 after round p's updates (as beside panel
// p in the barrier version), behind the wave's round count (kPfCountFirst);
// idle(4, 0, lane) on wave 0 after diag16(3), before the closing barrier.
//
// With the fold, wave 0's first apply and lookahead need only blocks (1, 0)
// and (1, 1) folded -- the first blocks waves 1 and 2 fold -- not the whole
// round 0 (wave 3's third block made wave 0 wait ~500 cycles after diag16(0)):
// those two count in *fcnt, and waves 1-3 await the complete round 0
// themselves before their first applies.
enum PotrfFlag {
  kPfPanel = 0,    // panels whose diagonal block is factored and next block applied: wave 0 sets (lds_set), waves
                   // 1-3 wait for it before panel p's applies
  kPfApplied = 1,  // applies done by waves 1-3, three increments per panel (lds_add); each of them waits for
                   // 3 (p + 1) before panel p's trailing updates
  kPfRound = 2,    // update rounds done by waves 1-3 (round 0 the fold, round p + 1 panel p's trailing updates),
                   // three increments per round (lds_add); wave 0 waits for 3 (p + 1) before its apply of panel p
  kPfCaller = 3,   // the caller's own count (k_factor_dag: thirds of its fused tile loaded), zeroed with the others
  kPfFlags = 4
};
// (*fcnt: blocks (1, 0) and (1, 1) of the fold done -- waves 1 and 2 add, wave 0 waits for 2; all four flags, *fcnt
// and *bad are zeroed by thread 0 before the start barrier)
//
// The round count and the side work (kPfCountFirst).  A wave's round count says that its share of the round's
// updates of D is done; wave 0 waits for it after diag16(p) and needs nothing of what idle(p) does.  Counted after
// idle(p) (0, the order this pipeline had), everything the caller does there -- loads it waits for, counter
// polls -- stands on wave 0's chain; counted before it (1), the side work has the next kPfPanel as a soft
// deadline instead.  No access of idle relies on the count coming after it:
//   * k_factor_dag's thirds are stored into X from idle(1) on, and X may hold the fold's operand F.  idle(1) comes
//     after lds_wait(fl + kPfPanel, 1), which wave 0 sets after its own fold block and diag16(0), and -- with the
//     early fold -- after lds_wait(fl + kPfRound, 3), every wave's count *behind* its fold blocks in either
//     order; without fcnt wave 0 itself waits for round 0 before it sets kPfPanel.
//   * its trsm_step(st) beside panel p reads LTd[st] and blocks (st, c), c < st <= p - 1, of D: final since
//     kPfPanel >= p and kPfApplied >= 3 p, which the wave awaited before the round's updates.  Wave 0, now up
//     to one panel ahead (it still needs round p + 1, counted after idle(p) returns), writes blocks (p + 1, p),
//     (p + 1, p + 1), inv and LTd[p + 1] meanwhile: none of those.
//   * what idle leaves in LDS for after the factorization is ordered by the closing barrier as before, and the
//     thirds by their own count (kPfCaller).
// The products and their order are the same either way.
#ifndef ARSLAM_PF_COUNT_FIRST
#define ARSLAM_PF_COUNT_FIRST 1
#endif
constexpr bool kPfCountFirst = ARSLAM_PF_COUNT_FIRST != 0;
//
// ws (a build with -DARSLAM_DAG_SUBSTAMPS only; else unused): kPsStamps words of global memory, or null, for
// wave 0's own s_memrealtime stamps (PfStamp), written by its lane 0 -- where wave 0 waits for waves 1-3
// (tools/potrf_cont.py).  k_factor_dag points it at the ticket's trace words and fills kPsIdle1 .. itself.
enum PfStamp {
  kPsWait0 = 0,   // .. + 5: wave 0 before (2p) and after (2p + 1) its wait for round p, p = 0 .. 2
  kPsClose = 6,   // wave 0 at the closing barrier (diag16(3) and idle(4, 0) done)
  kPsIdle1 = 7,   // .. + 2: the caller's: wave 1 + i back from idle(3) (the clock's low 32 bits)
  kPsStamps = 10
};
#ifdef ARSLAM_DAG_SUBSTAMPS
#define PF_WSTAMP(ws, i, lane)                                                                \
  do {                                                                                        \
    if (ws) {                                                                                 \
      __builtin_amdgcn_sched_barrier(0);                                                      \
      unsigned long long _t;                                                                  \
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");         \
      if ((lane) == 0) ((__attribute__((address_space(1))) unsigned long long *)(ws))[i] = _t;  \
      __builtin_amdgcn_sched_barrier(0);                                                      \
    }                                                                                         \
  } while (0)
#else
#define PF_WSTAMP(ws, i, lane) do {} while (0)
#endif
template <class Idle>
__device__ bool blocked_potrf64_async(double *D, double *inv, double *LTd, int *bad, int *fl, int tid,
                                      double *colx, Idle &&idle, const double *F = nullptr, bool fold = false,
                                      int *fcnt = nullptr, unsigned long long *ws = nullptr) {
  const int w = tid >> 6, lane = tid & 63;
  const bool early = fold && fcnt;
  if (tid == 0) {
    *bad = 0;
    fl[kPfPanel] = fl[kPfApplied] = fl[kPfRound] = fl[kPfCaller] = 0;
    if (fcnt) *fcnt = 0;
  }
  __syncthreads();
  if (w == 0) {
    STAMP(30);
    for (int p = 0; p < 4; ++p) {
      const int b0 = 16 * p;
      if (p == 0 && fold) wave_gemm16_sub(D, F, F, 64, lane);
      // (p > 0: block (p, p) had panel p-1's lookahead update at the end of
      // iteration p-1, and rounds 0 .. p-1 were awaited there)
      STAMP(31 + 6 * p);
      STAMP(32 + 6 * p);
      diag16(D, b0, inv, LTd + p * 16 * LI, bad, lane, colx);
      STAMP(33 + 6 * p);
      if (p < 3) {
        PF_WSTAMP(ws, kPsWait0 + 2 * p, lane);
        if (p == 0 && early) lds_wait(fcnt, 2);   // blocks (1, 0) and (1, 1) folded
        else lds_wait(fl + kPfRound, 3 * (p + 1));      // round p: block (p+1, p) has panel p-1's update
        PF_WSTAMP(ws, kPsWait0 + 2 * p + 1, lane);
        STAMP(34 + 6 * p);
        // The block below the diagonal solved transposed, Y = L_pp^{-1} A^T
        // (the same products as A L_pp^{-T}, operands swapped: bit-identical),
        // so each lane holds X[i][lk + 4 reg] -- the MFMA operand layout of
        // X X^T: the next diagonal block's lookahead update runs from the
        // registers, without reading X back from LDS.
        const int li = lane & 15, lk = lane >> 4;
        double *Cb = D + (b0 + 16) * LQ + b0, *Cd = Cb + 16;
        const double *Linv = LTd + p * 16 * LI;
        double a[4], cd[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = Cb[li * LQ + 4 * q + lk];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) cd[reg] = Cd[(lk + 4 * reg) * LQ + li];
        __builtin_amdgcn_wave_barrier();
        dbl4 y = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) y = __builtin_amdgcn_mfma_f64_16x16x4f64(Linv[li * LI + 4 * q + lk], a[q], y, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) Cb[li * LQ + lk + 4 * reg] = y[reg];
        lds_set(fl + kPfPanel, p + 1);
        STAMP(35 + 6 * p);
        dbl4 g = {0, 0, 0, 0};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) g = __builtin_amdgcn_mfma_f64_16x16x4f64(y[reg], y[reg], g, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) Cd[(lk + 4 * reg) * LQ + li] = cd[reg] - g[reg];
      }
    }
    idle(4, 0, lane);   // wave 0's own side work, diag16(3) done: waves 1-3 are still in idle(3)
    PF_WSTAMP(ws, kPsClose, lane);
  } else {
    if (fold) {
      // the fold's lower blocks 1..9 in row order (I, C), I >= C: (1,0) (1,1) (2,0) (2,1) ...
      for (int t = w; t < 10; t += 3) {
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        const int C = t - I * (I + 1) / 2;
        wave_gemm16_sub(D + 16 * I * LQ + 16 * C, F + 16 * I * LQ, F + 16 * C * LQ, 64, lane);
        if (early && t <= 2) lds_add(fcnt, lane);   // (1, 0) by wave 1, (1, 1) by wave 2
      }
    }
    if (kPfCountFirst) lds_add(fl + kPfRound, lane);
    idle(0, w, lane);
    if (!kPfCountFirst) lds_add(fl + kPfRound, lane);
    for (int p = 0; p < 3; ++p) {
      const int b0 = 16 * p;
      if (p == 0 && early) lds_wait(fl + kPfRound, 3);   // every block folded (wave 0 no longer awaits it)
      lds_wait(fl + kPfPanel, p + 1);             // L_pp's block inverse, block (p+1, p) applied
      if (w < 3 - p - 1 + 1 && p + 1 + w <= 3)   // blocks (p+2 .. 3, p): wave w takes p + 1 + w
        wave_apply_inv16(D + (b0 + 16 * (1 + w)) * LQ + b0, LTd + p * 16 * LI, lane);
      lds_add(fl + kPfApplied, lane);
      lds_wait(fl + kPfApplied, 3 * (p + 1));        // every block of panel p applied
      // panel p's update of blocks (I, C), I >= C >= p + 1, except (p + 1, p + 1)
      const int m = 3 - p, ntl = m * (m + 1) / 2;
      for (int t = w; t < ntl; t += 3) {
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        const int C = t - I * (I + 1) / 2;
        const int bi = 16 * (p + 1 + I), bc = 16 * (p + 1 + C);
        wave_gemm16_sub(D + bi * LQ + bc, D + bi * LQ + b0, D + bc * LQ + b0, 16, lane);
      }
      if (kPfCountFirst) lds_add(fl + kPfRound, lane);
      idle(p + 1, w, lane);
      if (!kPfCountFirst) lds_add(fl + kPfRound, lane);
    }
  }
  __syncthreads();
  return *bad == 0;
}

__device__ __forceinline__ bool blocked_potrf64(double *D, double *inv, double *LTd, int *bad, int tid, double *colx) {
  return blocked_potrf64_idle(D, inv, LTd, bad, tid, colx, [](int, int, int) {});
}

// Column step p of the blocked solve X L^T = A for row block rb of X (one
// wave): X[rb, p] -= X[rb, 0:p] L[p, 0:p]^T, then X[rb, p] <- X[rb, p] L_pp^{-T}.
__device__ __forceinline__ void trsm_step(double *X, const double *D, const double *LTd, int rb, int p, int lane) {
  const int b0 = 16 * p;
  if (p > 0) wave_gemm16_sub(X + 16 * rb * LQ + b0, X + 16 * rb * LQ, D + b0 * LQ, b0, lane);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  wave_apply_inv16(X + 16 * rb * LQ + b0, LTd + p * 16 * LI, lane);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// In-LDS blocked solve X L^T = A for a 64x64 tile X (256 threads), L from
// blocked_potrf64 (lower part of D, inv = 1 / diag).
__device__ __forceinline__ void blocked_trsm64(double *X, const double *D, const double *inv, const double *LTd,
                               int tid) {
  // row block w of X depends only on itself (and on D, LTd): the four
  // column steps need wave-local ordering only; one barrier at the end
  const int w = tid >> 6, lane = tid & 63;
  for (int p = 0; p < 4; ++p) trsm_step(X, D, LTd, w, p, lane);
  __syncthreads();
}

// Inverse X = L^{-1} of the 64x64 lower factor in D (after blocked_potrf64),
// built in LDS as its transpose XT (XT[c][r] = X[r][c]) from the 16x16
// diagonal-block inverses Li_p in LTd:  X_qq = Li_q,
//   X_pq = -Li_p sum_{r=q}^{p-1} L_pr X_rq   (p > q).
// Wave q owns column block q (three dependent 16x16 MFMA steps at most);
// its 16x16 scratch sits in a part of XT that stays structurally zero.
__device__ __forceinline__ void blocked_trinv64(const double *D, const double *LTd, double *XT, int tid) {
  const int q = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const double *Lq = LTd + q * 16 * LI;
#pragma unroll
  for (int e = 0; e < 4; ++e) {   // XT block (q,q) = Li_q^T
    const int idx = lane + 64 * e, i = idx >> 4, j = idx & 15;
    XT[(16 * q + j) * LQ + 16 * q + i] = (j <= i) ? Lq[i * LI + j] : 0.0;
  }
  double *scr = XT + (q == 0 ? 48 : 16 * q) * LQ;   // columns 0..15 of row block 3 (q=0) or q
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int p = q + 1; p < 4; ++p) {
    dbl4 acc = {0, 0, 0, 0};
    for (int r = q; r < p; ++r)
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const double a = D[(16 * p + li) * LQ + 16 * r + 4 * k4 + lk];
        const double b = XT[(16 * q + li) * LQ + 16 * r + 4 * k4 + lk];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
    // acc[reg] = M[lk + 4 reg][li]; scratch rows = M^T rows
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) scr[li * LQ + lk + 4 * reg] = acc[reg];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    dbl4 x = {0, 0, 0, 0};
    const double *Lp = LTd + p * 16 * LI;
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4)
      x = __builtin_amdgcn_mfma_f64_16x16x4f64(Lp[li * LI + 4 * k4 + lk], scr[li * LQ + 4 * k4 + lk], x, 0, 0, 0);
    // x[reg] = (Li_p M)[lk + 4 reg][li] = -X_pq[...]
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) XT[(16 * q + li) * LQ + 16 * p + lk + 4 * reg] = -x[reg];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// acc += A B^T for two 64x64 LDS tiles (pitch LQ), 4 waves x 32x32 on
// v_mfma_f64_16x16x4_f64: wave w owns rows 32 (w >> 1).., columns 32 (w & 1)..,
// acc[q] its 16x16 block (q >> 1, q & 1) in the f64 MFMA's C/D layout
// (col = lane & 15, row = (lane >> 4) + 4 reg): acc_pos below
__device__ __forceinline__ void gemm64_nt(const double *sA, const double *sB, int tid, dbl4 acc[4]) {
  const int w = tid >> 6, lane = tid & 63;
  const int r0 = (w >> 1) * 32, c0 = (w & 1) * 32;
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll 4
  for (int kk = 0; kk < T64 / 4; ++kk) {
    const int kc = kk * 4 + lk;
    const double a0 = sA[(r0 + li) * LQ + kc];
    const double a1 = sA[(r0 + 16 + li) * LQ + kc];
    const double b0 = sB[(c0 + li) * LQ + kc];
    const double b1 = sB[(c0 + 16 + li) * LQ + kc];
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[3], 0, 0, 0);
  }
}

// element acc[q][reg] of gemm64_nt's accumulators: its (row, col) in the 64x64 tile
__device__ __forceinline__ void acc_pos(int tid, int q, int reg, int &row, int &col) {
  const int w = tid >> 6, lane = tid & 63;
  row = (w >> 1) * 32 + (q >> 1) * 16 + (lane >> 4) + 4 * reg;
  col = (w & 1) * 32 + (q & 1) * 16 + (lane & 15);
}

}  // namespace

}  // namespace arslam
