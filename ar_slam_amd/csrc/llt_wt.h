// llt_wt.h -- how workgroups of the persistent executors (llt_dag.hip) hand
// tiles to each other inside one launch: the dependency-counter poll, the
// write-through (sc1) tile loads and stores, the bounded wait with its clock,
// and the fault record of a wait that gave up.
#pragma once

#include "llt_tile.h"

#include <climits>

namespace arslam {

namespace {

// How long a dependency wait may last before it counts as a device fault: 50
// ms of the 100 MHz s_memrealtime clock (read every 16 polls), far beyond any
// legitimate wait (a whole factorization is < 1 ms).  A time limit, not a poll
// count: the chain tasks poll every unit and the update tasks every 16, so
// with a count the chain task waiting downstream of a stuck update gave up
// first and was the one reported; with the clock the earliest wait gives up
// first, i.e. the stuck task itself (its fault record names its counter).
constexpr unsigned long long kWaitCapTicks = 5000000ull;   // 50 ms at 100 MHz
// the bound on the poll count as well (the clock read is 1 in 16 polls)
constexpr long kSpinCap = 1L << 22;
// the 100 MHz s_memrealtime clock (the waits' time limit and the trace's time stamps)
__device__ __forceinline__ unsigned long long realtime() {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
// The time a wait has been *running*: the clock is read every 16th poll and
// each interval counts at most kGapTicks (1 ms; 16 polls take microseconds),
// so a wave descheduled by preemption (the hardware saves the whole dispatch's
// waves and restores them later) does not count the time it was off the
// machine, and a producer preempted with it is not reported as stuck.
constexpr unsigned long long kGapTicks = 100000ull;   // 1 ms at 100 MHz
struct WaitTimer {
  unsigned long long last, run = 0;
  __device__ __forceinline__ WaitTimer() : last(realtime()) {}
  // true once the wait has run kWaitCapTicks (checked on every 16th poll) or kSpinCap polls
  __device__ __forceinline__ bool expired(long spins) {
    if (spins > kSpinCap) return true;
    if ((spins & 15) != 0) return false;
    const unsigned long long now = realtime(), d = now - last;
    last = now;
    run += d < kGapTicks ? d : kGapTicks;
    return run > kWaitCapTicks;
  }
};
// s_sleep units (64 cycles) between two polls of a dependency counter.  Every
// poll is a device-scope atomic performed at the memory side; with a few
// hundred update tasks waiting at once, polling every 64 cycles slowed the
// whole factorization (the chain's own loads and hand-offs queue behind the
// polls): cfg3 k_factor_dag 796 -> 757 us with the update tasks polling
// every 16 units, flat from 16 to 32, worse at 64 (tools/variant_bench.sh).
// The chain tasks (POTRF, TRSM) and the backward solve keep polling fast.
#ifndef ARSLAM_POLL_SLEEP
#define ARSLAM_POLL_SLEEP 16
#endif
constexpr int kPollSleep = ARSLAM_POLL_SLEEP;   // update tasks
#ifndef ARSLAM_CHAIN_SLEEP
#define ARSLAM_CHAIN_SLEEP 1
#endif
constexpr int kChainSleep = ARSLAM_CHAIN_SLEEP;   // POTRF / TRSM tasks
constexpr int kBsolveSleep = 1;    // k_bsolve_dag (its waits are all on the chain)

// Poll a dependency counter with an atomic read-modify-write (+0): counters
// are advanced by device-scope atomic adds, and an RMW is performed where
// those are, so it observes them on every XCD.  (A plain relaxed load was
// observed to spin forever on a counter another task had already advanced.)
__device__ __forceinline__ int ld_acquire_relaxed(int *p) {
  // compare-and-swap that never matches (counters are >= 0): returns the value
  // without a write, and cannot be folded into a plain load as an RMW of 0 is
  int v = INT_MIN;
  __hip_atomic_compare_exchange_strong(p, &v, INT_MIN, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return v;
}

// Tile hand-offs between workgroups of the persistent kernel use the
// write-through form (MI355X_MICROARCH.md, visibility): every published
// tile is stored sc1 (8-byte agent-scope relaxed atomic stores) and every
// load of a tile that another workgroup may write in this launch is an sc1
// load, so no release or acquire fence is needed around the counters.
__device__ __forceinline__ void st_wt(double *p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_wt(const double *p) {
  return __longlong_as_double((long long)__hip_atomic_load(
      reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// 16-byte write-through store / sc1 loads (inline asm: hipcc has no 16-byte
// atomic form).  Loads are issued in groups inside ONE asm statement that
// also waits for them (vmcnt(0)), so the compiler never sees an asm output
// before its data has arrived.
// (the trailing s_nop: a VALU write of the data VGPRs right after a 128-bit
// store may land before the store has read them, and hipcc does not pad an
// asm statement; MI355X hazard rule, cdna_hip_programming.md §5.7)
__device__ __forceinline__ void st_wt16(double *p, dbl2 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// eight 16-byte sc1 loads p[k] -> v[k], waited
__device__ __forceinline__ void ld_wt16x8(const double *const p[8], dbl2 v[8]) {
  asm volatile(
      "global_load_dwordx4 %0, %8, off sc1\n\t"
      "global_load_dwordx4 %1, %9, off sc1\n\t"
      "global_load_dwordx4 %2, %10, off sc1\n\t"
      "global_load_dwordx4 %3, %11, off sc1\n\t"
      "global_load_dwordx4 %4, %12, off sc1\n\t"
      "global_load_dwordx4 %5, %13, off sc1\n\t"
      "global_load_dwordx4 %6, %14, off sc1\n\t"
      "global_load_dwordx4 %7, %15, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
      : "memory");
}
// sixteen 16-byte sc1 loads p[k] -> v[k], waited
__device__ __forceinline__ void ld_wt16x16(const double *const p[16], dbl2 v[16]) {
  asm volatile(
      "global_load_dwordx4 %0, %16, off sc1\n\t"
      "global_load_dwordx4 %1, %17, off sc1\n\t"
      "global_load_dwordx4 %2, %18, off sc1\n\t"
      "global_load_dwordx4 %3, %19, off sc1\n\t"
      "global_load_dwordx4 %4, %20, off sc1\n\t"
      "global_load_dwordx4 %5, %21, off sc1\n\t"
      "global_load_dwordx4 %6, %22, off sc1\n\t"
      "global_load_dwordx4 %7, %23, off sc1\n\t"
      "global_load_dwordx4 %8, %24, off sc1\n\t"
      "global_load_dwordx4 %9, %25, off sc1\n\t"
      "global_load_dwordx4 %10, %26, off sc1\n\t"
      "global_load_dwordx4 %11, %27, off sc1\n\t"
      "global_load_dwordx4 %12, %28, off sc1\n\t"
      "global_load_dwordx4 %13, %29, off sc1\n\t"
      "global_load_dwordx4 %14, %30, off sc1\n\t"
      "global_load_dwordx4 %15, %31, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]),
        "=&v"(v[8]), "=&v"(v[9]), "=&v"(v[10]), "=&v"(v[11]), "=&v"(v[12]), "=&v"(v[13]), "=&v"(v[14]),
        "=&v"(v[15])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7]), "v"(p[8]),
        "v"(p[9]), "v"(p[10]), "v"(p[11]), "v"(p[12]), "v"(p[13]), "v"(p[14]), "v"(p[15])
      : "memory");
}
// 11 16-byte sc1 loads p[k] -> v[k] in one batch, waited
__device__ __forceinline__ void ld_wt16x11(const double *const p[11], dbl2 v[11]) {
  asm volatile(
      "global_load_dwordx4 %0, %11, off sc1\n\t"
      "global_load_dwordx4 %1, %12, off sc1\n\t"
      "global_load_dwordx4 %2, %13, off sc1\n\t"
      "global_load_dwordx4 %3, %14, off sc1\n\t"
      "global_load_dwordx4 %4, %15, off sc1\n\t"
      "global_load_dwordx4 %5, %16, off sc1\n\t"
      "global_load_dwordx4 %6, %17, off sc1\n\t"
      "global_load_dwordx4 %7, %18, off sc1\n\t"
      "global_load_dwordx4 %8, %19, off sc1\n\t"
      "global_load_dwordx4 %9, %20, off sc1\n\t"
      "global_load_dwordx4 %10, %21, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]), "=&v"(v[8]), "=&v"(v[9]), "=&v"(v[10])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7]), "v"(p[8]), "v"(p[9]), "v"(p[10])
      : "memory");
}
// 19 16-byte sc1 loads p[k] -> v[k] in one batch, waited
__device__ __forceinline__ void ld_wt16x19(const double *const p[19], dbl2 v[19]) {
  asm volatile(
      "global_load_dwordx4 %0, %19, off sc1\n\t"
      "global_load_dwordx4 %1, %20, off sc1\n\t"
      "global_load_dwordx4 %2, %21, off sc1\n\t"
      "global_load_dwordx4 %3, %22, off sc1\n\t"
      "global_load_dwordx4 %4, %23, off sc1\n\t"
      "global_load_dwordx4 %5, %24, off sc1\n\t"
      "global_load_dwordx4 %6, %25, off sc1\n\t"
      "global_load_dwordx4 %7, %26, off sc1\n\t"
      "global_load_dwordx4 %8, %27, off sc1\n\t"
      "global_load_dwordx4 %9, %28, off sc1\n\t"
      "global_load_dwordx4 %10, %29, off sc1\n\t"
      "global_load_dwordx4 %11, %30, off sc1\n\t"
      "global_load_dwordx4 %12, %31, off sc1\n\t"
      "global_load_dwordx4 %13, %32, off sc1\n\t"
      "global_load_dwordx4 %14, %33, off sc1\n\t"
      "global_load_dwordx4 %15, %34, off sc1\n\t"
      "global_load_dwordx4 %16, %35, off sc1\n\t"
      "global_load_dwordx4 %17, %36, off sc1\n\t"
      "global_load_dwordx4 %18, %37, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]), "=&v"(v[8]), "=&v"(v[9]), "=&v"(v[10]), "=&v"(v[11]), "=&v"(v[12]), "=&v"(v[13]), "=&v"(v[14]), "=&v"(v[15]), "=&v"(v[16]), "=&v"(v[17]), "=&v"(v[18])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7]), "v"(p[8]), "v"(p[9]), "v"(p[10]), "v"(p[11]), "v"(p[12]), "v"(p[13]), "v"(p[14]), "v"(p[15]), "v"(p[16]), "v"(p[17]), "v"(p[18])
      : "memory");
}
// A 64x64 tile g1 -> lds1 (and g2 -> lds2 if given) and a column's 16x16
// block inverses ltd_g -> LTd (1152 doubles): every sc1 load in flight at
// once, one round trip instead of one per array
__device__ __forceinline__ void load_tiles_ltd_wt(const double *__restrict__ g1, double *lds1,
                                                  const double *__restrict__ g2, double *lds2,
                                                  const double *__restrict__ ltd_g, double *LTd, int tid) {
  constexpr int kL = kLtdSize / 2;   // 16-byte elements of the block inverses (576)
  const double *p[19];
  dbl2 v[19];
  const int nt = g2 ? 16 : 8;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    p[q] = g1 + 2 * (q * 256 + tid);
    p[8 + q] = (g2 ? g2 : g1) + 2 * (q * 256 + tid);
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int e = tid + 256 * u;
    p[16 + u] = ltd_g + 2 * (e < kL ? e : 0);
  }
  if (g2) {
    ld_wt16x19(p, v);
  } else {
    const double *p11[11] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[16], p[17], p[18]};
    dbl2 v11[11];
    ld_wt16x11(p11, v11);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = v11[q];
#pragma unroll
    for (int u = 0; u < 3; ++u) v[16 + u] = v11[8 + u];
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    *reinterpret_cast<dbl2 *>(lds1 + r * LQ + c2) = v[q];
    if (nt == 16) *reinterpret_cast<dbl2 *>(lds2 + r * LQ + c2) = v[8 + q];
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int e = tid + 256 * u;
    if (e < kL) *reinterpret_cast<dbl2 *>(LTd + 2 * e) = v[16 + u];
  }
}
// Half a 64x64 tile (128 threads, t2 = 0..127: 16-byte element u * 128 + t2
// into v[u]) as sixteen sc1 loads, ISSUED ONLY -- the registers hold the data
// after ld_wt16x16_wait, and nothing may read them before (the caller keeps
// them untouched; the pair shares one address, the second at +2048 bytes).
__device__ __forceinline__ void ld_wt16x16_issue(const double *__restrict__ g, int t2, dbl2 v[16]) {
  const double *p[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) p[m] = g + 2 * (2 * m * 128 + t2);
  asm volatile(
      "global_load_dwordx4 %0, %16, off sc1\n\t"
      "global_load_dwordx4 %1, %16, off offset:2048 sc1\n\t"
      "global_load_dwordx4 %2, %17, off sc1\n\t"
      "global_load_dwordx4 %3, %17, off offset:2048 sc1\n\t"
      "global_load_dwordx4 %4, %18, off sc1\n\t"
      "global_load_dwordx4 %5, %18, off offset:2048 sc1\n\t"
      "global_load_dwordx4 %6, %19, off sc1\n\t"
      "global_load_dwordx4 %7, %19, off offset:2048 sc1\n\t"
      "global_load_dwordx4 %8, %20, off sc1\n\t"
      "global_load_dwordx4 %9, %20, off offset:2048 sc1\n\t"
      "global_load_dwordx4 %10, %21, off sc1\n\t"
      "global_load_dwordx4 %11, %21, off offset:2048 sc1\n\t"
      "global_load_dwordx4 %12, %22, off sc1\n\t"
      "global_load_dwordx4 %13, %22, off offset:2048 sc1\n\t"
      "global_load_dwordx4 %14, %23, off sc1\n\t"
      "global_load_dwordx4 %15, %23, off offset:2048 sc1\n\t"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]), "=&v"(v[8]), "=&v"(v[9]), "=&v"(v[10]), "=&v"(v[11]), "=&v"(v[12]), "=&v"(v[13]), "=&v"(v[14]), "=&v"(v[15])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
      : "memory");
}
__device__ __forceinline__ void ld_wt16x16_wait(dbl2 v[16]) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15])::"memory");
}
// eight 8-byte sc1 loads, waited
__device__ __forceinline__ void ld_wt8x8(const double *const p[8], double v[8]) {
  asm volatile(
      "global_load_dwordx2 %0, %8, off sc1\n\t"
      "global_load_dwordx2 %1, %9, off sc1\n\t"
      "global_load_dwordx2 %2, %10, off sc1\n\t"
      "global_load_dwordx2 %3, %11, off sc1\n\t"
      "global_load_dwordx2 %4, %12, off sc1\n\t"
      "global_load_dwordx2 %5, %13, off sc1\n\t"
      "global_load_dwordx2 %6, %14, off sc1\n\t"
      "global_load_dwordx2 %7, %15, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
      : "memory");
}

// 256-thread sc1 load of a 64x64 row-major tile into LDS (pitch LQ)
__device__ __forceinline__ void load_tile_wt(const double *__restrict__ g, double *lds, int tid) {
  const double *p[8];
  dbl2 v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) p[q] = g + 2 * (q * 256 + tid);
  ld_wt16x8(p, v);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    *reinterpret_cast<dbl2 *>(lds + r * LQ + c2) = v[q];
  }
}

// two tiles at once (both sets of sc1 loads in flight before either is stored)
__device__ __forceinline__ void load_two_tiles_wt(const double *__restrict__ g1, double *lds1,
                                                  const double *__restrict__ g2, double *lds2, int tid) {
  const double *p[16];
  dbl2 v[16];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    p[q] = g1 + 2 * (q * 256 + tid);
    p[8 + q] = g2 + 2 * (q * 256 + tid);
  }
  ld_wt16x16(p, v);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    *reinterpret_cast<dbl2 *>(lds1 + r * LQ + c2) = v[q];
    *reinterpret_cast<dbl2 *>(lds2 + r * LQ + c2) = v[8 + q];
  }
}

// NT-thread write-through store of a 64x64 LDS tile (pitch LQ), optionally
// lower triangle only
template <int NT = 256>
__device__ __forceinline__ void store_tile_wt(double *__restrict__ g, const double *lds, int tid, bool lower) {
#pragma unroll
  for (int q = 0; q < 2048 / NT; ++q) {
    const int e = q * NT + tid, r = e >> 5, c2 = (e & 31) * 2;
    dbl2 v = *reinterpret_cast<const dbl2 *>(lds + r * LQ + c2);
    if (lower) {
      if (c2 > r) v.x = 0.0;
      if (c2 + 1 > r) v.y = 0.0;
    }
    st_wt16(g + 2 * e, v);
  }
}

// NE elements (16 bytes each, from element e0 on) of an LDS tile by NT threads,
// every LDS read of the thread issued before its first store.  st_wt16 is a
// compiler barrier, so in store_tile_wt's loop each read waits behind the store
// before it: one LDS round trip per element, in sequence.  (k_factor_dag's
// chain stores only: the other users of store_tile_wt keep their code.)
template <int NT, int NE>
__device__ __forceinline__ void store_elems_wt(double *__restrict__ g, const double *lds, int e0, int tid, bool lower) {
  dbl2 v[NE / NT];
#pragma unroll
  for (int q = 0; q < NE / NT; ++q) {
    const int e = e0 + q * NT + tid, r = e >> 5, c2 = (e & 31) * 2;
    v[q] = *reinterpret_cast<const dbl2 *>(lds + r * LQ + c2);
    if (lower) {
      if (c2 > r) v[q].x = 0.0;
      if (c2 + 1 > r) v[q].y = 0.0;
    }
  }
#pragma unroll
  for (int q = 0; q < NE / NT; ++q) st_wt16(g + 2 * (e0 + q * NT + tid), v[q]);
}

// wave 0: spin until counter[idx] >= val for every wait; false on timeout,
// or at once when another workgroup already timed out (flag < 0), so a
// broken graph drains in one spin cap instead of one per task.  Lane q polls
// wait q (64 at a time), so a task's counters are read in one round trip, not
// one after another.
// On a timeout *unmet = {counter, value seen, value awaited} of the first
// wait still unmet (uniform over the wave), for the fault record; *expired:
// this wait ran out of time (false: it gave up because another one had).
__device__ bool dag_wait(int *counters, const int2 *waits, int w0, int w1, int *flag, int lane, bool chain,
                         int3 *unmet, bool *expired) {
  for (int base = w0; base < w1; base += 64) {
    const int w = base + lane;
    const bool mine = w < w1;
    const int2 cv = mine ? waits[w] : make_int2(0, 0);
    long spins = 0;
    WaitTimer tm;
    for (;;) {
      // (every lane re-polls each round: no loop-carried per-lane state)
      const int got = mine ? ld_acquire_relaxed(counters + cv.x) : 0;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(mine && got < cv.y);
      if (m == 0) break;
      if (chain) __builtin_amdgcn_s_sleep(kChainSleep);
      else __builtin_amdgcn_s_sleep(kPollSleep);
      const bool exp = tm.expired(++spins);
      const bool give_up = exp || ((spins & 255) == 0 && __builtin_amdgcn_readfirstlane(ld_acquire_relaxed(flag)) < 0);
      if (give_up) {
        *expired = exp;
        const int l = __builtin_ctzll(m);
        *unmet = make_int3(__builtin_amdgcn_readlane(cv.x, l), __builtin_amdgcn_readlane(got, l),
                           __builtin_amdgcn_readlane(cv.y, l));
        return false;
      }
    }
  }
  return true;
}

// A wait of ticket t gave up (one thread): raise the launch's fault flag
// (-(kind * 1000000 + t)); the workgroup whose code wins it also fills the
// fault record (kDagFault*), which the host reads to name the stuck counter,
// its producers and how far the launch had drawn.  Plain agent-scope atomic
// stores: the record is read after the launch.
// Every wait that ran out of time (not one that gave up after another's
// fault) also records its ticket in kFaultFirstStuck (as INT_MAX - ticket,
// max-combined): the smallest stuck ticket, where a stuck chain starts.
__device__ void dag_fault(int *flag, int *counters, int n_tiles, const int *ticket, int kind, int t, int3 unmet,
                          bool expired) {
  int *f = counters + 2 * n_tiles + kDagOffFault;
  if (expired) __hip_atomic_fetch_max(f + kFaultFirstStuck, INT_MAX - t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (atomicCAS(flag, 0, -(kind * 1000000 + t)) != 0) return;
  const int v[kFaultFirstStuck] = {t, kind, unmet.x, unmet.y, unmet.z,
                                   ld_acquire_relaxed(const_cast<int *>(ticket)),
                                   ld_acquire_relaxed(counters + 2 * n_tiles + kDagOffInflight), (int)blockIdx.x};
#pragma unroll
  for (int i = 0; i < kFaultFirstStuck; ++i)   // (kFaultFirstStuck itself is max-combined above)
    __hip_atomic_store(f + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// all threads: drain this workgroup's write-through stores before thread 0
// bumps a counter
__device__ __forceinline__ void dag_release(int tid) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

}  // namespace

}  // namespace arslam
