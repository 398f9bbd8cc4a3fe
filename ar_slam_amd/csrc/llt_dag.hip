// llt_dag.hip -- Cholesky of the reduced (tag + camera) system on gfx950,
// replacing the Eigen::LLT that Ceres' DenseSchurComplementSolver runs on one
// CPU thread.
//
// Storage: compact 64 x 64 fp64 tiles (only the tiles of the factor exist;
// tile (i,j) at S + tile_id[i*T+j] * 4096, assembled tiles first so the
// multi-GPU all-reduce of the Schur sums covers one contiguous prefix).
// Right-looking tiled factorization driven by a tile plan (LltPlan):
//   for k:  POTRF(k,k)            one wavefront, lane r owns row r in VGPRs
//           TRSM (i,k)            one wavefront per tile, rows in VGPRs,
//                                 L_kk^T in LDS (broadcast reads)
//           UPDATE (i,j)          A_ij -= L_ik L_jk^T on MFMA
//                                 (v_mfma_f64_16x16x4_f64, 4 waves x 32x32)
// The plan lists, per step k, the tiles the step touches.  A dense plan lists
// every lower tile; a sparse plan lists only the tiles of the symbolic
// Cholesky fill of the reduced system (tile level), so a structurally zero
// tile is never read or written.  A skipped update would have added exactly
// 0 (products with an all-zero tile), so the sparse plan computes the same
// factor as the dense plan on the same ordering.
//
// The right-hand side rides along as row nF of the matrix (inside the padded
// last tile row), so the forward substitution L z = b falls out of the
// factorization; the backward solve L^T y = z is one launch per tile row.
//
// Two executors run this: one launch per level of the plan (llt_levels.hip)
// and the persistent task-graph kernels of this file (k_factor_dag,
// k_bsolve_dag), with the launchers and resets that go with them.  Both are
// built from the tile primitives of llt_tile.h; the hand-offs between the
// workgroups of one launch are in llt_wt.h.
#include "llt_tile.h"
#include "llt_wt.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace arslam {

namespace {

// ---------------------------------------------------------------------------
// Persistent task-graph executor of the same factorization.  Every workgroup
// loops: draw a ticket (tasks are in a topological order, dag_build), wait
// (thread 0, bounded spin) for the task's dependency counters, run it, and
// publish its result (stores drained, agent-scope release, counter update).
// A waited-on task always holds a smaller ticket, i.e. it was drawn by a
// running workgroup, so progress is guaranteed for any grid size; every
// spin is still bounded (kSpinCap) and raises the error flag if exceeded.
//   POTRF k   : L_kk and L_kk^{-1} into Ld (the column's TRSMs then need
//               only a GEMM with the inverse)
//   TRSM i,k  : L_ik = A_ik L_kk^{-T}  (MFMA, in place)
//   update    : the plan item's sum over its columns k of L_ik L_jk^T; split
//               items publish partials and the last arriver reduces them in
//               chunk order; the application to the target waits for the
//               target's earlier levels, so the summation order is fixed.
// ---------------------------------------------------------------------------
// The first panel beside which the fused solve's steps may run (4: never).
// cfg3 k_factor_dag: 3 -> 660.8, 4 -> 665.1, 2 -> 676.1, 1 -> 683.8 us
// (interleaved, one box): waves 1-3 working beside the earlier panels slow
// wave 0's diagonal blocks (the same steps alone on the chip cost nothing,
// tools/pipe_bench.hip).  Measured again with the round counted before the
// side work and row block 3 on wave 0 (profiles/potrf_sidework/): 3 -> 558.2,
// 2 -> 556.5, 1 -> 557.2 us, inside the spread of two copies of one library.
#ifndef ARSLAM_PIPE_FROM
#define ARSLAM_PIPE_FROM 3
#endif
constexpr int kPipeFrom = ARSLAM_PIPE_FROM;
#ifndef ARSLAM_PIPE_W2
#define ARSLAM_PIPE_W2 0
#endif
// The wave that takes row block 3's early steps: 1-3 beside the last panel after its own row block's, or 0: wave 0
// itself once the last diagonal block is factored, beside the other waves' steps.
constexpr int kPipeW2 = ARSLAM_PIPE_W2;

struct DagArgs {
  double *S;
  int T;
  double *Ld;                 // [2T][4096]: L_kk then L_kk^{-1}
  double *ltd;                // [T][kLtdSize]: the 16x16 diagonal-block inverses of each L_kk
  // (the task, its fused TRSM, continuation, fold and update-item fields are
  // all in the ticket's record; LltPlan::dag_rec)
  const int *rec;             // [n_tasks][32] each ticket's record (DagRecField)
  const int2 *ks_tiles;       // [ks] operand tile ids of an update column
  const int *ks;              // [ks] the column of each (a multi-column fold's own term test)
  int *claimed;               // [n_tasks] continuation targets: claimed by the predecessor or the drawer
  const int2 *waits;          // wait lists {counter, value} (ranges in the records)
  int *counters;              // ready[n_tiles] | applied[n_tiles] | ticket
  int n_tiles;
  int n_tasks;
  double *part;
  int *split_cnt;
  int *flag;
  int t_begin, t_end;         // this launch's tickets (one phase of a multi-rank plan, or all)
  int *ticket;                // its ticket counter
  int *progress;              // debug: [grid][kDagProgressInts] host-visible (DagProgressSlot)
  unsigned long long *trace;  // debug: [n_tasks][kDagTraceWords] s_memrealtime stamps (DagTraceWord)
  // tiles >= first_store are fill tiles the Schur gather does not write -- S
  // never clears them, and their first update stores 0 - acc instead of
  // reading the tile (INT_MAX: every tile is cleared and read-modify-written)
  int first_store;
  int *started;               // workgroups of this launch that have started (the claim cap's base)
  int wg_limit;               // debug: workgroups with blockIdx.x >= wg_limit return at once (INT_MAX: none)
};

// A ticket's 32-int record: two scalar loads in flight, one wait (the record
// array is read-only in the launch).  From LDS for a claimed continuation
// (its predecessor copied it there beside its POTRF).
typedef int int16v __attribute__((ext_vector_type(16)));
struct DagRecV {
  int16v a, b;
  __device__ __forceinline__ int operator[](int i) const { return i < 16 ? a[i] : b[i - 16]; }
};
__device__ __forceinline__ DagRecV load_rec(const int *p) {
  DagRecV r;
  asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
               : "=s"(r.a), "=s"(r.b)
               : "s"(p)
               : "memory");
  return r;
}
__device__ __forceinline__ DagRecV lds_rec(const int *s) {
  DagRecV r;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    r.a[i] = __builtin_amdgcn_readfirstlane(s[i]);
    r.b[i] = __builtin_amdgcn_readfirstlane(s[16 + i]);
  }
  return r;
}

// k_factor_dag's workgroup protocol: int slots in LDS behind LTd, then the
// claimed continuation's record.  Who writes a slot, who reads it, and what
// orders the two -- "barrier": a __syncthreads() between the store and the
// loads; "flag": the slot is the hand-off itself (lds_set / lds_add / lds_wait,
// llt_tile.h).  Slots 5, 19, 22 and 23 are free (19, 22, 23: a stamped build's exit times of waves 1-3).
enum DagShSlot {
  kShTicket = 0,      // thread 0: the ticket it drew; all, between the two barriers at the top of the loop
  kShBad = 1,         // blocked_potrf64_async's `bad`: its waves 0 (diag16); all, after its closing barrier
  kShRun = 2,         // wave 0 lane 0: this workgroup runs the ticket (a claimed target, or drawn and not claimed
                      // by its predecessor); all, after the barrier that ends the early wait
  kShLast = 3,        // update item, thread 0: first "the target's in-order wait was met at the first fetch", then
                      // "this split piece arrived last"; all, after the barrier that follows each store
  kShClaim = 4,       // POTRF task, thread 0: the continuation ticket it claimed, or -1; all, after the task's
                      // last barrier (the next loop round starts from it)
  kShFetchReq = 6,    // fused tile: wave 1 lane 0 stores the panel beside which it saw the late waits met (-1:
                      // panel 0); waves 1-3 read it beside the later panels (volatile LDS accesses, no ordering
                      // needed: a stale 0 only postpones the fetch); reset by thread 0 before the POTRF's start barrier
  kShFoldCnt = 7,     // blocked_potrf64_async's fcnt (flag: waves 1-2 add, wave 0 waits)
  kShPipe0 = 8,       // .. + 3: blocked_potrf64_async's fl[kPf*] (flags; reset at its start barrier)
  kShThirds = 11,     // = fl[kPfCaller]: thirds of the fused tile in X (flag: waves 1-3 add beside the panels and
                      // wait beside the last one); read plainly after the POTRF's closing barrier
  kShSolveStep0 = 12, // .. + 3: column steps of the fused solve already applied to row block b beside the last
                      // panel: the lane 0 of the wave that ran them; wave b, after the barrier before the solve;
                      // reset by thread 0 before the POTRF's start barrier
  kShAkkHalf0 = 16,   // .. + 1: waves 2-3 lane 0: their half of the continuation's A_kk is in D; the continuation
                      // (next loop round), barriers between
  kShTake = 18,       // beside the last panel, wave 1's decision for waves 1-3 (flag: 1 take the thirds, 2 skip);
                      // reset by thread 0 before the POTRF's start barrier
  kShContMet0 = 20,   // .. + 1: waves 2-3 lane 0: the continuation's early waits seen met beside the last panel;
                      // all, after the POTRF's closing barrier
  kShRec = 24,        // .. + kDagRecInts: the claimed continuation's record: wave 3 beside panel 2; lds_rec at the
                      // top of the next loop round, barriers between
  kShInts = kShRec + kDagRecInts
};
static_assert(kShThirds == kShPipe0 + kPfCaller && kShPipe0 + kPfFlags <= kShSolveStep0, "the POTRF pipeline's flags");
static_assert(kShContMet0 + 1 < kShRec && kShInts % 2 == 0, "the slots fit before the record; colx stays 8-byte aligned");

#define DAG_PROGRESS(slot, v)                                                                  \
  do {                                                                                         \
    if (a.progress && tid == 0)                                                                \
      __hip_atomic_store(a.progress + kDagProgressInts * blockIdx.x + (slot), (v), __ATOMIC_RELAXED,          \
                         __HIP_MEMORY_SCOPE_SYSTEM);                                            \
  } while (0)

// The trace's stamps between a POTRF's two publishes (kTrSolveTop .. kTrAcked,
// tools/potrf_cont.py) exist only in a build with -DARSLAM_DAG_SUBSTAMPS
// (ARSLAM_EXTRA_FLAGS): as run-time debug code like the other stamps they
// reallocate the kernel (110 spilled SGPRs against 107), and at 256 VGPRs an
// allocation is worth 1-4 %; the stretch is measured on a build of
// its own and the library's kernel does not depend on them.
#ifdef ARSLAM_DAG_SUBSTAMPS
#define DAG_SUBSTAMP(word)                                                                      \
  do {                                                                                          \
    if (a.trace && tid == 0) a.trace[kDagTraceWords * (long)t + (word)] = realtime();           \
  } while (0)
#else
#define DAG_SUBSTAMP(word) do {} while (0)
#endif

__global__ __launch_bounds__(256, kDagWorkgroupsPerCu) void k_factor_dag(DagArgs a) {
  // one LDS array carved per task type (POTRF: D, X, inv, LTd; GEMMs: sA, sB)
  // D | X | inv | LTd | the protocol's slots and record (DagShSlot) | colx
  __shared__ __attribute__((aligned(16))) double lds[2 * T64 * LQ + T64 + kLtdSize + kShInts / 2 + T64];
  double *D = lds, *X = lds + T64 * LQ, *inv = X + T64 * LQ, *LTd = inv + T64;
  int *sh = reinterpret_cast<int *>(LTd + kLtdSize);
  int *sh_rec = sh + kShRec;                    // the claimed continuation's record
  double *colx = LTd + kLtdSize + kShInts / 2;   // POTRF pivot scratch (X stays free for the prefetch)
  int *ready = a.counters, *applied = a.counters + a.n_tiles, *ticket = a.ticket;
  // claimed continuation targets in flight.  A target is claimed once its
  // EARLY waits are all drawn; its late waits may name undrawn tickets, so at
  // most half the grid may hold claimed targets: the other workgroups can
  // always draw the lowest unfinished ticket, whose producers are all done.
  //
  // "Half the grid" is not enough when fewer workgroups than the grid are
  // resident (another process on the GPU, several ranks sharing one): every
  // resident workgroup could then hold a claimed target while the ones that
  // would draw never start.  So the cap is half the workgroups that have
  // *started* (counted on entry, read at each claim): a started workgroup
  // stays resident until every ticket is drawn, so at least half of the
  // started ones hold no claimed target and can draw the lowest unfinished
  // ticket (dag_simulate's started-k schedules).
  int *inflight = a.counters + 2 * a.n_tiles + kDagOffInflight;
  if ((int)blockIdx.x >= a.wg_limit) return;   // (debug: only wg_limit workgroups ever start)
  if (threadIdx.x == 0) __hip_atomic_fetch_add(a.started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // Per-CU "POTRF running" flags (performance only: a wrong or stale flag
  // costs a bounded pause, never a result).  The 64x64 POTRF is a chain of
  // dependent LDS/VALU steps on one wave; the other workgroup on its CU runs
  // update GEMMs that take SIMD issue and LDS bandwidth from it (the POTRF
  // phase takes ~11 us in the contended half of the factorization, 8.5
  // beside idle neighbours), so updates on that CU hold their next GEMM
  // (at most ~55 us) while the flag is up: cfg3 k_factor_dag 689 -> ~675 us.
  // A flag held across the POTRF task's late wait made it 2x slower (the
  // wait can need an update the flag holds).
  int *cu_flag = a.counters + 2 * a.n_tiles + kDagOffCuFlags;
  int cu_key = 0;
  {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    cu_key = (int)(((xcc & 7u) << 8) | ((hw >> 8) & 0xffu));   // XCC, SE, SH, CU
  }
  // Continuation targets stay ordinary tickets with a claim flag.  The
  // predecessor's workgroup claims its target (before publishing the tile the
  // target waits for, so it wins whenever it claims) if every task the target
  // waits on has been drawn -- then the target only waits on running tasks --
  // and runs it at once, the folded tile still in LDS.  Otherwise the
  // workgroup that drew the target claims and runs it once its waits are met.
  int next = -1, prev_k = -1;
  bool next_met = false;   // a claimed continuation whose early waits were already seen met
  // DEAD: fast_next is never set, so `fast` below is always false and its three
  // `!fast` guards always pass.  They are what is left of the fast continuation
  // (removed) and stay on purpose: taking them out changes no
  // result but makes hipcc allocate the whole kernel anew (122 SGPR spills
  // against 107), and that build measured 4 % slower on cfg3 (616 against 592
  // us, profiles/llt_split/README.md).  Remove them only with a measurement.
  bool fast_next = false;
  for (;;) {
    // thread coordinates re-derived per task from a laundered threadIdx: the
    // per-lane LDS/tile addresses of every task type are then computed where
    // they are used instead of being hoisted out of the loop and spilled
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int w = tid >> 6, lane = tid & 63;
    const int r0 = (w >> 1) * 32, c0 = (w & 1) * 32;
    const int li = lane & 15, lk = lane >> 4;
    const bool cont = next >= 0;
    if (!cont) {
      if (tid == 0) sh[kShTicket] = a.t_begin + atomicAdd(ticket, 1);
      __syncthreads();
      next = sh[kShTicket];
      __syncthreads();
    }
    const int t = __builtin_amdgcn_readfirstlane(next);
    const int pk = prev_k;   // a claimed continuation: the predecessor's column (its L_{k,pk} is in X)
    const bool premet = cont && next_met;   // (only for the claimed target it was polled for)
    const bool fast = cont && fast_next;
    next = -1;
    prev_k = -1;
    next_met = false;
    fast_next = false;
    DAG_PROGRESS(kProgTicket, t);
    DAG_PROGRESS(kProgPhase, 1);
    if (t >= a.t_end) break;
    const DagRecV r = cont ? lds_rec(sh_rec) : load_rec(a.rec + (long)t * kDagRecInts);
    const int4 task = make_int4(r[kRecType], r[kRecY], r[kRecZ], r[kRecW]);
    DAG_PROGRESS(kProgType, task.x);
    if (a.trace && tid == 0) { a.trace[kDagTraceWords * (long)t + kTrDraw] = realtime(); a.trace[kDagTraceWords * (long)t + kTrWg] = blockIdx.x; }
    const int2 sub = make_int2(r[kRecSub], r[kRecLate]);
    if (w == 0) {
      // (sub.y: the end of the early waits; the late ones are a fused TRSM's,
      // or a folded TRSM's L_kk)
      int3 unmet;
      bool expired = false;
      const bool ok =
          premet || dag_wait(a.counters, a.waits, r[kRecWait0], sub.y, a.flag, lane, task.x != 2, &unmet, &expired);
      if (lane == 0) {
        if (!ok) dag_fault(a.flag, a.counters, a.n_tiles, ticket, 1, t, unmet, expired);   // stuck ticket, for diagnosis
        // a drawn continuation target: run it only if its predecessor did not claim it
        sh[kShRun] = (cont || r[kRecMaxdep] < 0 || atomicCAS(a.claimed + t, 0, 1) == 0) ? 1 : 0;
      }
    }
    if (!fast) {
      __syncthreads();
      if (!sh[kShRun]) continue;
    }
    DAG_PROGRESS(kProgPhase, 2);
    if (a.trace && tid == 0) a.trace[kDagTraceWords * (long)t + kTrMet] = realtime();
    // the chain tasks (POTRF, TRSM) win SIMD arbitration over co-resident updates
    if (task.x != 2) __builtin_amdgcn_s_setprio(3);
    if (task.x == 0) {
      // ---- POTRF k: publish L_kk and its 16x16 block inverses, then (off the
      // critical path) the full inverse for the backward solve ----
      const int k = task.y;
      // The continuation's A_kk, prefetched by waves 2-3 into registers beside
      // the last POTRF panel once its early waits are met (apf: the target
      // folds this task's solved tile alone, so A_kk is all it loads).  Waves
      // 2-3 wait for those loads right after the solve anyway (they move the
      // registers into D, as the target's A_kk), before the wait for their
      // share of the solved tile's stores: the release never waits for them.
      const int c = sub.x >= 0 ? r[kRecCont] : -1;
      const int apf_tile = sub.x >= 0 ? r[kRecContAkk] : -1;
      const bool apf = apf_tile >= 0;
      const double *apf_src = a.S + (long)max(apf_tile, 0) * (T64 * T64);
      bool ap_met = false;   // waves 2-3: the target's early waits seen met beside the last panel
      int c_rec = 0;         // wave 3 (lanes 0-31): the target's record, bound for sh_rec
      int2 c_wait = make_int2(0, 0);   // waves 2-3: lane q's early wait of the target
      dbl2 apv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) apv[u] = dbl2{0.0, 0.0};
      bool ap_ok = false;
      // this CU's flag is up from the fold to the end of the factorization,
      // never across a wait (an update held on this CU may be what a wait
      // needs; the early waits are met here, the late ones come after)
      if (tid == 0)
        __hip_atomic_store(cu_flag + cu_key, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int4 fit = make_int4(0, r[kRecQ0], r[kRecQ1], 0);
      const bool akk_in_d = cont && sh[kShAkkHalf0] && sh[kShAkkHalf0 + 1];   // (its predecessor's waves 2-3 put A_kk in D)
      // a one-column folded update runs inside the factorization (fold_f: its
      // L_kj tile in X -- the predecessor's solved tile for a continuation,
      // else loaded beside A_kk); several columns fold first, as one GEMM pass
      const bool fold_in = task.z >= 0 && fit.z - fit.y == 1;
      if (fold_in) {
        const double *Akk = a.S + (long)task.w * (T64 * T64);
        if (cont && r[kRecFoldK0] == pk) {
          if (!akk_in_d) load_tile_wt(Akk, D, tid);
        } else load_two_tiles_wt(Akk, D, a.S + (long)r[kRecFoldTile0] * (T64 * T64), X, tid);
      } else if (task.z >= 0) {
        // folded final update: A_kk -= sum over the item's columns j of L_kj L_kj^T
        const int4 it = fit;
        dbl4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        // A_kk (final: the task's waits are met) straight into the MFMA
        // accumulator layout, sc1 loads in flight during the fold's GEMMs
        double akk[16];
        {
          const double *Akk = a.S + (long)task.w * (T64 * T64);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rb = r0 + (q >> 1) * 16, cb = c0 + (q & 1) * 16;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) akk[4 * q + reg] = ld_wt(Akk + (rb + lk + 4 * reg) * T64 + cb + li);
          }
        }
        // (the same products in the same order whether the task was drawn
        // or claimed: a claimed continuation takes the term of its
        // predecessor's column from the tile that task just solved, still in X)
        for (int q = it.y; q < it.z; ++q) {
          if (cont && a.ks[q] == pk) {
            gemm64_nt(X, X, tid, acc);
            continue;
          }
          if (q > it.y) __syncthreads();
          load_tile_wt(a.S + (long)a.ks_tiles[q].x * (T64 * T64), D, tid);
          __syncthreads();
          gemm64_nt(D, D, tid, acc);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rb = r0 + (q >> 1) * 16, cb = c0 + (q & 1) * 16;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) D[(rb + lk + 4 * reg) * LQ + cb + li] = akk[4 * q + reg] - acc[q][reg];
        }
      } else {
        load_tile_wt(a.S + (long)task.w * (T64 * T64), D, tid);
      }
      if (!fast) __syncthreads();
      if (a.trace && tid == 0) a.trace[kDagTraceWords * (long)t + kTrLoaded] = realtime();
      // The fused TRSM's tile: wave 1 fetches it into X while wave 0 factors
      // the first diagonal block, if its late waits are already met;
      // otherwise it is waited for and loaded after L_kk is published.
      const double *pf_src = sub.x >= 0 ? a.S + (long)sub.x * (T64 * T64) : nullptr;
      const int pw0 = sub.y, pw1 = r[kRecWait1];
      // lane q's late wait of the fused tile (loaded now, polled beside the panels)
      const int2 pw_wait = (sub.x >= 0 && pw0 + lane < pw1) ? a.waits[pw0 + lane] : make_int2(0, 0);
      // A tile whose waits were not met at panel 0 is polled again by wave 1
      // beside panels 1 and 2 (the request in kShFetchReq) and fetched by waves 1-3,
      // a third each, beside the next panel: on the late elimination-tree chain
      // the tile's last update lands a few microseconds into the POTRF
      // (cfg3 k_factor_dag 758 -> 736 us).
      if (tid == 0 && !fast) {   // (a fast continuation: reset by its predecessor)
        sh[kShFetchReq] = 0;
        sh[kShSolveStep0] = sh[kShSolveStep0 + 1] = sh[kShSolveStep0 + 2] = sh[kShSolveStep0 + 3] = 0;   // the fused solve's column steps done per row block
        sh[kShTake] = 0;   // beside the last panel: wave 1's take / skip (1 / 2)
      }
      // kShThirds: thirds of the tile loaded into X (3: all; set to 0 by the
      // pipeline's start).  Each wave decides for its own third: a wave that
      // reaches a panel late must not take another wave's completed third for
      // the whole tile.
      bool third_done = false;
      // The fused solve's first steps beside the last panel: once the whole
      // tile is in X, waves 1-3 apply the solve's column steps 0-2 while wave 0
      // factors the last diagonal block (wave w takes row block w - 1), so only
      // step 3 remains after the factorization (the same products in the same
      // order).  Row block 3's steps are wave 0's own, once that block is
      // factored (kPipeW2 == 0): on a second wave they came behind that wave's
      // own row block, 48 dependent MFMAs in a row, and wave 0 stood 2.4 us at
      // the closing barrier on every prefetched link -- its three round waits
      // together are 0.2 us (profiles/potrf_sidework/stretch_parent.txt).  Now
      // the four waves reach the barrier within 0.2 us of each other.  Beside
      // the earlier panels the steps slow the factorization more than they
      // save (kPipeFrom).
      int sdone = 0;
#ifdef ARSLAM_DAG_SUBSTAMPS
      // the waves' own stamps inside the POTRF (PfStamp) go straight to the ticket's trace words (zeroed by the host)
      unsigned long long *const ws = a.trace ? a.trace + kDagTraceWords * (long)t + kTrPfStamp0 : nullptr;
#else
      unsigned long long *const ws = nullptr;
#endif
      const bool ok = blocked_potrf64_async(D, inv, LTd, sh + kShBad, sh + kShPipe0, tid, colx, [&](int p, int wv, int ln) {
        if (wv == 0) {
          // wave 0, the last diagonal block factored (p == 4): row block 3's steps 0-2 (kPipeW2 == 0), if the
          // tile is in X by now -- else wave 3 runs them after the barrier, as without the prefetch
          if (kPipeW2 == 0 && kPipeFrom <= 3 && pf_src && lds_get(sh + kShThirds) >= 3) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            for (int st = 0; st < 3; ++st) trsm_step(X, D, LTd, 3, st, ln);
            if (ln == 0) sh[kShSolveStep0 + 3] = 3;
          }
          return;
        }
        auto fetch_third = [&]() {
        auto poll = [&]() {
          if (!pf_src || pw1 - pw0 > 64) return false;
          const int q = pw0 + ln;
          const int got = q < pw1 ? ld_acquire_relaxed(a.counters + pw_wait.x) : 0;
          return __builtin_amdgcn_ballot_w64(q < pw1 && got < pw_wait.y) == 0;
        };
        int lnl = ln;   // laundered: the prefetch addresses are formed here, not hoisted and spilled
        asm volatile("" : "+v"(lnl));
        if (p == 0) {   // (X may still hold the fold's operand: the thirds go out beside panel 1)
          if (wv == 1 && poll() && ln == 0) *as_lds(sh + kShFetchReq) = -1;
          return;
        }
        if (third_done || lds_get(sh + kShThirds) >= 3) return;
        const int req = lds_get(sh + kShFetchReq);
        // not requested yet: wave 1 polls beside panels 1 and 2, and beside the
        // last panel for all three waves (kShTake); each then takes its own third
        bool take = req != 0 && req < p;
        if (req == 0) {
          if (p < 3) {
            if (wv == 1 && poll() && ln == 0) *as_lds(sh + kShFetchReq) = p;
          } else {
            // one decision for waves 1-3 (wave 1 polls), so that a wave that
            // takes its third knows the other two do as well
            if (!pf_src || pw1 - pw0 > 64) {
              take = false;
            } else if (wv == 1) {
              take = poll();
              lds_set(sh + kShTake, take ? 1 : 2);
            } else {
              lds_wait(sh + kShTake, 1);
              take = lds_get(sh + kShTake) == 1;
            }
          }
        }
        if (take) {   // the three thirds, one batch of sc1 loads each
          // 2048 16-byte elements of the 64x64 tile: wave w takes e in [(w-1)*683, min(w*683, 2048))
          const int e0 = (wv - 1) * 683, e1 = min(wv * 683, 2048);
          const double *p11[11];
          dbl2 v[11];
#pragma unroll
          for (int u = 0; u < 11; ++u) p11[u] = pf_src + 2 * min(e0 + u * 64 + lnl, e1 - 1);
          ld_wt16x11(p11, v);
#pragma unroll
          for (int u = 0; u < 11; ++u) {
            const int e = e0 + u * 64 + ln, r = e >> 5, c2 = (e & 31) * 2;
            if (e < e1) *reinterpret_cast<dbl2 *>(X + r * LQ + c2) = v[u];
          }
          third_done = true;
          lds_add(sh + kShThirds, ln);
        }
        };
        // (beside the last panel the continuation's counters are read first,
        // so their round trip overlaps the fused tile's)
        int c_got = 0;
        bool c_mine = false;
        if (p == 3 && c >= 0 && wv >= 2 && r[kRecContLate] - r[kRecContWait0] <= 64) {
          const int q = r[kRecContWait0] + ln;
          c_mine = q < r[kRecContLate] && c_wait.x != sub.x;   // (the tile this task solves counts as met)
          if (c_mine) c_got = ld_acquire_relaxed(a.counters + c_wait.x);
        }
        fetch_third();
        // waves 2-3 and the continuation target: its record into LDS (wave 3,
        // issued beside panel 1, stored beside panel 2), its early-wait list
        // (beside panel 2) and their counters (beside panel 3, where wave 0
        // waits for nothing from them): loads in flight across a panel, so no
        // round trip delays an update round wave 0 waits for
        if (c >= 0 && wv >= 2) {
          const int cw0 = r[kRecContWait0], cw1 = r[kRecContLate];
          if (p == 1 && wv == 3 && ln < kDagRecInts) c_rec = a.rec[(long)c * kDagRecInts + ln];
          if (p == 2) {
            if (wv == 3 && ln < kDagRecInts) sh_rec[ln] = c_rec;
            const int q = cw0 + ln;
            if (q < cw1) c_wait = a.waits[q];
          }
          if (p == 3) {
            const bool met = cw1 - cw0 <= 64 && __builtin_amdgcn_ballot_w64(c_mine && c_got < c_wait.y) == 0;
            if (ln == 0) sh[kShContMet0 + wv - 2] = met ? 1 : 0;
            ap_met = met && apf;
          }
        }
        // beside the last panel every wave that took its third waits for the
        // other two (they took theirs too), so the solve's steps 0-2 always run
        // here once the tile is in, not only when all thirds landed by chance
        // (cfg3 k_factor_dag 605.9 -> 601.3 us, cfg2 207.1 -> 205.6, same-box A/B)
        if (p == 3 && third_done && sdone < 3) lds_wait(sh + kShThirds, 3);
        if (kPipeFrom <= 3 && pf_src && p >= kPipeFrom && sdone < p && lds_get(sh + kShThirds) >= 3) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          for (int st = sdone; st < p; ++st) {
            trsm_step(X, D, LTd, wv - 1, st, ln);
            if (wv == kPipeW2) trsm_step(X, D, LTd, 3, st, ln);
          }
          sdone = p;
          if (ln == 0) {
            sh[kShSolveStep0 + wv - 1] = sdone;
            if (wv == kPipeW2) sh[kShSolveStep0 + 3] = sdone;
          }
        }
#ifdef ARSLAM_DAG_SUBSTAMPS
        // back from the last panel's side work: the clock's low word into a free slot (19, 22, 23), thread 0
        // copies it to the trace after the closing barrier (a 64-bit store from here spills an eighth VGPR)
        if (p == 3 && ln == 0) *as_lds(sh + (wv == 1 ? 19 : 20 + wv)) = (int)realtime();
#endif
      }, X, fold_in, sh + kShFoldCnt, ws);   // (fold_in, not a null test of the LDS pointer: hipcc mis-selects that null check)
      // A fused solve whose tile is already in X has no wait: the CU's flag
      // stays up through it too (the solve is the link's next stretch of the
      // chain; cfg3 k_factor_dag 621.9 -> 604.2 us, same-box A/B)
      const bool keep_flag = sub.x >= 0 && sh[kShThirds] >= 3;
      if (tid == 0 && !keep_flag)
        __hip_atomic_store(cu_flag + cu_key, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.trace && tid == 0) a.trace[kDagTraceWords * (long)t + kTrFactored] = realtime();
#ifdef ARSLAM_DAG_SUBSTAMPS
      if (a.trace && tid == 0) {
        a.trace[kDagTraceWords * (long)t + kTrPfStamp0 + kPsIdle1] = (unsigned)sh[19];
        a.trace[kDagTraceWords * (long)t + kTrPfStamp0 + kPsIdle1 + 1] = (unsigned)sh[22];
        a.trace[kDagTraceWords * (long)t + kTrPfStamp0 + kPsIdle1 + 2] = (unsigned)sh[23];
      }
#endif
      if (!ok && tid == 0) {
        int first = 0;
        while (first < T64 && D[first * LQ + first] > 0.0) ++first;
        atomicCAS(a.flag, 0, 1 + k * T64 + first);
      }
      double *ltd_g = a.ltd + (long)k * kLtdSize;
      // (Measured slower: L_kk stored by one wave and released beside the
      // solve or by the continuation -- the other TRSMs of the column, on the
      // path to the continuation's fused tile, then start later.)
      store_tile_wt(a.Ld + (long)k * T64 * T64, D, tid, true);
      for (int e = tid; e < kLtdSize / 2; e += 256)
        st_wt16(ltd_g + 2 * e, *reinterpret_cast<const dbl2 *>(LTd + 2 * e));
      dag_release(tid);
      if (tid == 0) __hip_atomic_fetch_add(ready + task.w, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.trace && tid == 0) a.trace[kDagTraceWords * (long)t + kTrPublished] = realtime();
      if (sub.x >= 0) {
        // fused TRSM of the parent's tile against the L_kk still in LDS
        const bool pref = sh[kShThirds] >= 3;   // (written inside the POTRF, barriers since)
        if (!pref) {
          if (w == 0) {
            int3 unmet;
            bool expired = false;
            const bool ok2 = dag_wait(a.counters, a.waits, sub.y, r[kRecWait1], a.flag, lane, true, &unmet, &expired);
            if (!ok2 && lane == 0) dag_fault(a.flag, a.counters, a.n_tiles, ticket, 3, t, unmet, expired);
          }
          __syncthreads();
        }
        double *Ct = a.S + (long)sub.x * (T64 * T64);
        // The continuation claim's round trips ride along the solve instead of
        // following it: the ticket count and the in-flight reservation go out
        // now, the claim itself after the solve, answered during the tile's
        // stores (its target's early waits were polled beside the last POTRF
        // panel, kShContMet0..1: a claimed target whose waits were seen met skips
        // its own poll).
        int tk_seen = 0, infl_old = 0, started_seen = 0;
        if (c >= 0 && tid == 0) {
          tk_seen = ld_acquire_relaxed(ticket);
          started_seen = ld_acquire_relaxed(a.started);
          infl_old = atomicAdd(inflight, 1);
        }
        if (!pref) load_tile_wt(Ct, X, tid);
        if (ap_met) {   // waves 2-3: the continuation's A_kk in flight during the solve
          int t2 = tid - 128;
          asm volatile("" : "+v"(t2));
          ld_wt16x16_issue(apf_src, t2, apv);
          ap_ok = true;
        }
        __syncthreads();
        DAG_SUBSTAMP(kTrSolveTop);
        // blocked_trsm64, its steps inline (row block w per wave), from the
        // first step not applied beside the last panel
        const int s0 = pref ? sh[kShSolveStep0 + w] : 0;
        for (int st = s0; st < 2; ++st) trsm_step(X, D, LTd, w, st, lane);
        // claim the continuation target before the tile is published: its
        // drawer waits for this tile, so it cannot have claimed it yet.  (The
        // CAS goes out here and is answered beside the last two steps.)
        const bool want = c >= 0 && tid == 0 && a.t_begin + tk_seen > r[kRecContMaxdep] && infl_old < started_seen / 2;
#ifdef ARSLAM_DAG_SUBSTAMPS
        if (a.trace && tid == 0) asm volatile("" ::"v"(tk_seen), "v"(started_seen), "v"(infl_old));   // (the prelude's answers are in)
#endif
        DAG_SUBSTAMP(kTrWantKnown);
        int cas_old = 1;
        if (want) cas_old = atomicCAS(a.claimed + c, 0, 1);
        for (int st = max(s0, 2); st < 4; ++st) trsm_step(X, D, LTd, w, st, lane);
        // every wave stores the row block it solved (no other wave wrote it)
        // as soon as its own steps are done, its LDS reads in one batch; the
        // acknowledgements come in beside the barrier and the A_kk move
        store_elems_wt<64, 512>(Ct, X, 512 * w, lane, false);
        if (keep_flag && tid == 0)
          __hip_atomic_store(cu_flag + cu_key, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        DAG_SUBSTAMP(kTrSolved);
        // waves 2-3 move the continuation's A_kk into D (free: L_kk's last
        // reader was the solve)
        if (w >= 2) {
          if (ap_ok) {
            ld_wt16x16_wait(apv);
            const int t2 = tid - 128;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
              const int e = u * 128 + t2, row = e >> 5, c2 = (e & 31) * 2;
              *reinterpret_cast<dbl2 *>(D + row * LQ + c2) = apv[u];
            }
          }
          if (lane == 0) sh[kShAkkHalf0 + w - 2] = ap_ok ? 1 : 0;
        }
        if (tid == 0) {
          const int claim = want && cas_old == 0 ? c : -1;
          if (c >= 0 && claim < 0) atomicSub(inflight, 1);
          sh[kShClaim] = claim;
        }
        // (every wave waits for its own stores' acknowledgements: waves 2-3
        // have waited for A_kk by now, thread 0 for the claim's answer;
        // releasing the tile from the continuation instead was measured slower)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        DAG_SUBSTAMP(kTrAcked);
        if (tid == 0) __hip_atomic_fetch_add(ready + sub.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a.trace && tid == 0) {
          a.trace[kDagTraceWords * (long)t + kTrSubPublished] = realtime();
          // (debug flags above the workgroup: premet, A_kk prefetched into D, fused tile prefetched,
          // the continuation's early waits seen met, claimed)
          const unsigned long long fl = (premet ? 1 : 0) | (akk_in_d ? 2 : 0) | (pref ? 4 : 0) |
                                        (sh[kShContMet0] && sh[kShContMet0 + 1] ? 8 : 0) | (sh[kShClaim] >= 0 ? 16 : 0);
          a.trace[kDagTraceWords * (long)t + kTrWg] = blockIdx.x | (fl << 32);
        }
        __syncthreads();
        next = sh[kShClaim];
        next_met = next >= 0 && sh[kShContMet0] && sh[kShContMet0 + 1];
        if (next >= 0) prev_k = k;
      } else if (r[kRecInv] > 0) {
        // the root column: no fused tile, no continuation, and no INV task --
        // L_kk and its block inverses are still in D and LTd, X is free, so the
        // inverse is formed here (the INV branch's products in its order: the
        // same bits) instead of closing the launch with a task that reloads them
        blocked_trinv64(D, LTd, X, tid);
        __syncthreads();
        double *Xg = a.Ld + ((long)a.T + k) * T64 * T64;
        // (fully unrolled, where the INV branch unrolls by 4: with this loop at
        // 1, 2, 4 or 8 the kernel spills an eighth VGPR, 36 B of scratch per lane)
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          const int e = m * 256 + tid, row = e >> 6, col = e & 63;
          Xg[e] = (row >= col) ? X[col * LQ + row] : 0.0;   // read by the next kernel only
        }
      }
    } else if (task.x == 3) {
      // ---- INV k: L_kk^{-1} for the backward solve (off the critical chain) ----
      const int k = task.y;
      load_tiles_ltd_wt(a.Ld + (long)k * T64 * T64, D, nullptr, nullptr, a.ltd + (long)k * kLtdSize, LTd, tid);
      __syncthreads();
      blocked_trinv64(D, LTd, X, tid);
      __syncthreads();
      double *Xg = a.Ld + ((long)a.T + k) * T64 * T64;
#pragma unroll 4
      for (int m = 0; m < 16; ++m) {
        const int e = m * 256 + tid, r = e >> 6, c = e & 63;
        Xg[e] = (r >= c) ? X[c * LQ + r] : 0.0;   // read by the next kernel only
      }
    } else if (task.x == 1) {
      // ---- TRSM i,k: L_ik L_kk^T = A_ik, blocked with the 16x16 inverses ----
      const int k = task.z;
      double *Ct = a.S + (long)task.w * (T64 * T64);
      // the tile, L_kk and its block inverses in one round trip
      load_tiles_ltd_wt(Ct, X, a.Ld + (long)k * T64 * T64, D, a.ltd + (long)k * kLtdSize, LTd, tid);
      __syncthreads();
      if (a.trace && tid == 0) a.trace[kDagTraceWords * (long)t + kTrLoaded] = realtime();
      blocked_trsm64(X, D, inv, LTd, tid);
      if (a.trace && tid == 0) a.trace[kDagTraceWords * (long)t + kTrFactored] = realtime();
      store_tile_wt(Ct, X, tid, false);
      dag_release(tid);
      if (tid == 0) __hip_atomic_fetch_add(ready + task.w, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      // ---- update item ----
      const int4 it = make_int4(0, r[kRecQ0], r[kRecQ1], r[kRecSid]);
      const int ti = r[kRecTi], tj = r[kRecTj], sid = it.w;
      dbl4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
      // The target's in-order wait (its earlier levels applied) is polled
      // beside the first operand fetch; when it is met then, the target's own
      // loads go out before the last GEMM and land during it (one round trip
      // fewer after the GEMM).  (Unsplit items: a split piece stores a partial.)
      double *C = a.S + (long)task.w * (T64 * T64);
      double cv[16];
      bool c_pre = false;
      if (task.z == 0 && task.w >= a.first_store) {   // (0 - acc below: the same bits)
#pragma unroll
        for (int u = 0; u < 16; ++u) cv[u] = 0.0;
        c_pre = true;
      }
      for (int q = it.y; q < it.z; ++q) {
        // (operand tile ids: the first column's in the record, no column -> tile lookup chain)
        const int2 kt = q == it.y ? make_int2(r[kRecTile0I], r[kRecTile0J]) : a.ks_tiles[q];
        if (q > it.y) __syncthreads();
        {   // hold the GEMM while a POTRF runs on this CU (bounded)
          if (tid == 0) {
            for (int spin = 0; spin < 256 &&
                               __hip_atomic_load(cu_flag + cu_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                 ++spin)
              __builtin_amdgcn_s_sleep(8);
          }
          __syncthreads();
        }
        if (q == it.y && sid < 0 && tid == 0)
          sh[kShLast] = (task.z == 0 || ld_acquire_relaxed(applied + task.w) >= task.z) ? 1 : 0;
        if (ti != tj)   // both operands in one round trip
          load_two_tiles_wt(a.S + (long)kt.x * (T64 * T64), D, a.S + (long)kt.y * (T64 * T64), X, tid);
        else
          load_tile_wt(a.S + (long)kt.x * (T64 * T64), D, tid);
        __syncthreads();
        const bool c_issue = q == it.z - 1 && sid < 0 && sh[kShLast] && !c_pre;
        if (c_issue) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int rb = r0 + (u >> 1) * 16, cb = c0 + (u & 1) * 16;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) cv[4 * u + reg] = ld_wt(C + (rb + lk + 4 * reg) * T64 + cb + li);
          }
          c_pre = true;
        }
        gemm64_nt(D, ti != tj ? X : D, tid, acc);   // a diagonal target: one operand tile, fetched once
      }
      bool apply = true;
      if (sid >= 0) {
        const int2 sp = make_int2(r[kRecSplitN], r[kRecSplitP]);
        double *mine = a.part + (long)(sp.y + (sid & 255)) * 4096;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) st_wt(mine + (4 * q + reg) * 256 + tid, acc[q][reg]);
        dag_release(tid);
        if (tid == 0) {
          const int old = __hip_atomic_fetch_add(a.split_cnt + (sid >> 8), 1, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
          sh[kShLast] = old == sp.x - 1;
        }
        __syncthreads();
        apply = sh[kShLast] != 0;
        if (apply) {
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] = dbl4{0, 0, 0, 0};
          for (int c = 0; c < sp.x; ++c) {
            const double *pc = a.part + (long)(sp.y + c) * 4096;
            double v[16];
            const double *p8[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) p8[u] = pc + u * 256 + tid;
            ld_wt8x8(p8, v);
            ld_wt8x8(p8 + 8, v + 8);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) acc[q][reg] += v[4 * q + reg];
          }
        }
      }
      DAG_PROGRESS(kProgPhase, 3);
      if (apply && !c_pre) {
        // in level order: wait until the target's earlier levels were applied
        if (tid == 0) {
          long spins = 0;
          int seen;
          WaitTimer tm;
          while ((seen = ld_acquire_relaxed(applied + task.w)) < task.z) {
            __builtin_amdgcn_s_sleep(kPollSleep);
            const bool exp = tm.expired(++spins);
            if (exp || (((spins & 255) == 0) && ld_acquire_relaxed(a.flag) < 0)) {
              dag_fault(a.flag, a.counters, a.n_tiles, ticket, 2, t, make_int3(a.n_tiles + task.w, seen, task.z), exp);
              break;
            }
          }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // (sixteen loads in flight)
          const int rb = r0 + (q >> 1) * 16, cb = c0 + (q & 1) * 16;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) cv[4 * q + reg] = ld_wt(C + (rb + lk + 4 * reg) * T64 + cb + li);
        }
      }
      if (apply) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rb = r0 + (q >> 1) * 16, cb = c0 + (q & 1) * 16;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            st_wt(C + (rb + lk + 4 * reg) * T64 + cb + li, cv[4 * q + reg] - acc[q][reg]);
        }
        dag_release(tid);
        if (tid == 0) __hip_atomic_fetch_add(applied + task.w, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    DAG_PROGRESS(kProgPhase, 4);
    if (cont && tid == 0) atomicSub(inflight, 1);   // this claimed target is done
    __builtin_amdgcn_s_setprio(0);
    if (a.trace && tid == 0) a.trace[kDagTraceWords * (long)t + kTrEnd] = realtime();
  }
  {
    const int tid = threadIdx.x;
    DAG_PROGRESS(kProgPhase, 9);
  }
}

// Persistent backward solve L^T y = z (the launch-per-level pair above as one
// launch).  Ticket b takes column bs_cols[b]; the columns are root level
// first, so every ancestor a column waits for holds an earlier ticket and was
// drawn by a running workgroup (deadlock-free for any grid).  A column task:
//   z_k      from the rhs row (as k_init_z), loaded at the top of the task
//            beside X_kk: nothing it needs depends on the gathers;
//   gathers  nearest ancestor LAST (ancestors finish root-first, so all but
//            the parent's partial are summed while the parent is still being
//            solved), y_i is an sc1 load (written this launch), and the
//            partials are summed in this fixed order, so every rank of a
//            sharded solve computes the same bits;
//   solve    y_k = L_kk^{-T}(z_k - acc) with the prefetched inverse X_kk;
//            wave 0 stores y_k write-through, drains, bumps done[k].
// The gather loop is software-pipelined so that no load whose address depends
// on another load sits between a parent's y and the column's own y:
//   - the plan stores each gathered tile's compact index (gtile[g] =
//     tile_id[i*T+k]), so an item's operands are {gather[g].x, gtile[g]} and
//     the 16 L_ik values per thread: two round trips, not three;
//   - the ticket is made wave-uniform (readfirstlane), so the plan's arrays
//     are read with scalar loads: they are counted apart from the vector
//     loads and never stand in front of a poll;
//   - item g-1's L_ik values are issued into the second register set (lvA /
//     lvB, swapped by unrolling the loop twice: no moves) right after the
//     FIRST poll load of y_i of item g, and the indices of item g-2 with
//     them.  Vector loads return in order, so a prefetch issued before that
//     first load would hold every poll back; issued after it, its one round
//     trip runs beside the poll's own -- and on the root path y_i is a whole
//     link away when item g starts.  (Chosen over an inline-asm poll with a
//     counted wait: that form needs every prefetch load in asm and counted by
//     hand as well.  The compiler barrier pins the order.  ISA, per item:
//     global_load_dwordx2 sc1 of y, 16 global_load_dwordx2, two s_load_dword,
//     then the poll loop, whose compare hipcc guards with s_waitcnt vmcnt(0):
//     the first compare of an item waits for its prefetch too, so an item
//     costs at least one L_ik round trip -- one, where the dependent fetch
//     was three -- and that trip is hidden whenever y_i is not there yet.)
//   No prefetch reads outside the column's range [gbeg[b], gbeg[b+1]): the
//   index loads are clamped to it and the last item issues no L_ik loads.  A
//   timed-out wait leaves the task with its prefetched registers unused.
__device__ __forceinline__ void bs_issue_lik(const double *__restrict__ S, int tile, int w, int lane,
                                             double (&lv)[16]) {
  const double *Lik = S + (long)tile * (T64 * T64);
#pragma unroll
  for (int m = 0; m < 16; ++m) lv[m] = Lik[(w + 4 * m) * T64 + lane];   // rows w, w+4, ..., lane's column
}

__global__ __launch_bounds__(256) void k_bsolve_dag(const double *__restrict__ S, const int *__restrict__ tid_map,
                                                    int T, const double *__restrict__ Ld, long nR,
                                                    const int *__restrict__ cols, const int2 *__restrict__ gather,
                                                    const int *__restrict__ gtile, const int *__restrict__ gbeg,
                                                    int ncols, double *yF, int *counters, int *flag) {
  __shared__ double red[4][T64];
  __shared__ double ys[T64];
  enum { kBsTicket, kBsOk, kBsSlots };   // thread 0: the drawn ticket; wave 0 lane 0: the item's wait did not give up
  __shared__ int sh[kBsSlots];           // (both read by all after the barrier that follows the store)
  if (*flag) return;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  int *ticket = counters + T;   // (counters[0..T) are unused: y entries are their own flags)
  const double *Xinv = Ld + (long)T * T64 * T64;
  const long kr = nR / T64;
  for (;;) {
    if (tid == 0) sh[kBsTicket] = atomicAdd(ticket, 1);
    __syncthreads();
    const int b = __builtin_amdgcn_readfirstlane(sh[kBsTicket]);
    if (b >= ncols) break;
    const int k = cols[b];
    const int g0 = gbeg[b], g1 = gbeg[b + 1];
    const long row0 = (long)k * T64;
    // the inverse's rows 16w..16w+15 for lane's column, in flight during the gathers
    const double *X = Xinv + (long)k * T64 * T64;
    double xv[16];
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) xv[rr] = X[(16 * w + rr) * T64 + lane];
    double z = 0.0;   // wave 0: lane's entry of z_k
    if (w == 0 && row0 + lane < nR) {
      if (k == kr) z = Ld[kr * T64 * T64 + (nR - kr * T64) * T64 + lane];
      else z = tile_ptr(S, tid_map, T, (int)kr, k)[(nR - kr * T64) * T64 + lane];
    }
    double acc = 0.0;   // wave 0: lane's row of sum_i L_ik^T y_i
    // the pipeline's state: item g is the current one (ancestor i_cur, its
    // L_ik in flight or landed in one of lvA / lvB), {i_nxt, t_nxt} are item
    // g-1's ancestor and tile
    double lvA[16], lvB[16];
    int g = g1 - 1, i_cur = 0, i_nxt = 0, t_nxt = 0;
    if (g >= g0) {
      i_cur = gather[g].x;
      bs_issue_lik(S, gtile[g], w, lane, lvA);
      const int gn = max(g - 1, g0);
      i_nxt = gather[gn].x;
      t_nxt = gtile[gn];
    }
    // one item: lv holds its L_ik, lvn takes the next item's; false = the wait gave up
    auto item = [&](double (&lv)[16], double (&lvn)[16]) -> bool {
      const long ri = (long)i_cur * T64;
      // y_i is its own ready flag: the entries are kYSentinel until column
      // i's task stores them (8-byte write-through stores, never torn), so
      // the wait is the load itself -- no counter, no drain before it
      double yv = 0.0;
      bool mine = w == 0 && ri + lane < nR;
      if (mine) yv = ld_wt(yF + ri + lane);
      asm volatile("" ::: "memory");   // (the first poll load is issued; now the prefetch)
      if (g > g0) bs_issue_lik(S, t_nxt, w, lane, lvn);
      const int gnn = max(g - 2, g0);
      const int i_nn = gather[gnn].x, t_nn = gtile[gnn];
      if (w == 0) {
        bool ok = true;
        long spins = 0;
        WaitTimer tm;
        for (;;) {
          if (mine) mine = (unsigned long long)__double_as_longlong(yv) == kYSentinel;
          if (__builtin_amdgcn_ballot_w64(mine) == 0) break;
          __builtin_amdgcn_s_sleep(kBsolveSleep);
          if (tm.expired(++spins) || (((spins & 255) == 0) &&
                                     __builtin_amdgcn_readfirstlane(ld_acquire_relaxed(flag)) != 0)) {
            if (lane == 0) atomicCAS(flag, 0, -(4000000 + b));
            ok = false;
            break;
          }
          if (mine) yv = ld_wt(yF + ri + lane);
        }
        if (lane == 0) sh[kBsOk] = ok;
        ys[lane] = (ri + lane < nR) ? yv : 0.0;
      }
      __syncthreads();
      if (!sh[kBsOk]) return false;
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < 16; ++m) s += lv[m] * ys[w + 4 * m];
      red[w][lane] = s;
      __syncthreads();
      if (w == 0) acc += ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
      i_cur = i_nxt;
      i_nxt = i_nn;
      t_nxt = t_nn;
      --g;
      return true;
    };
    while (g >= g0) {
      if (!item(lvA, lvB)) break;
      if (g < g0) break;
      if (!item(lvB, lvA)) break;
    }
    if (w == 0) ys[lane] = (row0 + lane < nR) ? z - acc : 0.0;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) s += xv[rr] * ys[16 * w + rr];
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && row0 + lane < nR)   // (published by the store itself; see the gathers)
      st_wt(yF + row0 + lane, ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
  }
}

// tests only: copy the diagonal factors L_kk into their S tiles
__global__ void k_scatter_diag(double *__restrict__ S, const int *__restrict__ tid_map, int T,
                               const double *__restrict__ Ld) {
  const int k = blockIdx.x;
  double *t = tile_ptr(S, tid_map, T, k, k);
  for (int e = threadIdx.x; e < T64 * T64; e += blockDim.x) t[e] = Ld[(long)k * T64 * T64 + e];
}

}  // namespace

void launch_scatter_diag(const LltPlan &P, double *S, hipStream_t s) {
  hipLaunchKernelGGL(k_scatter_diag, dim3((unsigned)P.T), dim3(256), 0, s, S, P.tile_id, P.T, P.ldiag);
}

namespace {
// One launch zeroing the persistent executors' counters (and the step's
// failure flag) instead of a fill launch per array.
// (with ld.n > 0 also the step's LM diagonal: k_lm_diag's work, one launch less)
__global__ void k_exec_reset(int *flag, int *a, long na, int *b, long nb, int *c, long nc, int *d, long nd,
                             LmDiagArgs ld) {
  const long n = na + nb + nc + nd;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < ld.nys; e += (long)gridDim.x * blockDim.x)
    ld.ysent[e] = __longlong_as_double((long long)kYSentinel);
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n + ld.n; e += (long)gridDim.x * blockDim.x) {
    if (e < na) a[e] = 0;
    else if (e < na + nb) b[e - na] = 0;
    else if (e < na + nb + nc) c[e - na - nb] = 0;
    else if (e < n) d[e - na - nb - nc] = 0;
    else {
      const long i = e - n;
      const double v = ld.scale[i] * ld.scale[i] * ld.colnorm[i];   // squared column norm of J diag(s)
      ld.diag[i] = fmin(fmax(v, ld.dmin), ld.dmax);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
}
}  // namespace

void launch_exec_reset(const LltPlan &P, int *flag, hipStream_t s, const LmDiagArgs *ld) {
  const ExecReset r = exec_reset_args(P, flag, nullptr, 0);
  LmDiagArgs l{};
  if (ld) l = *ld;
  const long n = std::max(r.na + r.nb + r.nc + r.nd + l.n, l.nys);
  const unsigned grid = (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, 1024));
  hipLaunchKernelGGL(k_exec_reset, dim3(grid), dim3(256), 0, s, flag, r.a, r.na, r.b, r.nb, r.c, r.nc, r.d, r.nd, l);
}

ExecReset exec_reset_args(const LltPlan &P, int *flag, double *ysent, long nys) {
  ExecReset r;
  r.flag = flag;
  r.na = P.n_dag_tasks ? 2 * P.n_tiles + kDagCounterExtra : 0;
  r.a = P.dag_counters;
  r.nb = P.n_dag_tasks;
  r.b = P.dag_claimed;
  r.nc = P.n_split;
  r.c = P.upd_cnt;
  r.nd = P.h_bcols.empty() ? 0 : (long)P.T + 1;
  r.d = P.bs_counters;
  r.ysent = ysent;
  r.nys = nys;
  return r;
}

void launch_zero_tiles(const LltPlan &P, double *S, hipStream_t s) {
  if (P.n_tiles) (void)hipMemsetAsync(S, 0, (size_t)P.n_tiles * T64 * T64 * sizeof(double), s);
}

static int g_dag_wg_limit = INT_MAX;   // debug (arslam_debug_dag_workgroup_limit), process-wide
void set_dag_workgroup_limit(int k) { g_dag_wg_limit = k > 0 ? k : INT_MAX; }

void launch_dense_llt_dag(const LltPlan &P, double *S, int *flag, hipStream_t s, int n_workgroups, int *progress,
                          unsigned long long *trace, bool reset, int phase, long first_store) {
  const int t_begin = phase == 1 ? (int)P.phase_split : 0;
  const int t_end = phase == 0 ? (int)P.phase_split : (int)P.n_dag_tasks;
  if (t_end <= t_begin) return;
  if (reset) {
    (void)hipMemsetAsync(P.dag_counters, 0, (2 * (size_t)P.n_tiles + kDagCounterExtra) * sizeof(int), s);
    (void)hipMemsetAsync(P.dag_claimed, 0, (size_t)P.n_dag_tasks * sizeof(int), s);
    if (P.n_split) (void)hipMemsetAsync(P.upd_cnt, 0, P.n_split * sizeof(int), s);
  }
  int *extra = P.dag_counters + 2 * P.n_tiles;   // the counters after ready | applied (kDagOff*)
  DagArgs a;
  a.S = S;
  a.T = P.T;
  a.Ld = P.ldiag;
  a.ltd = P.ldiag + 2L * P.T * T64 * T64;
  a.rec = P.dag_rec;
  a.ks_tiles = P.dag_ks_tiles;
  a.ks = P.upd_ks;
  a.claimed = P.dag_claimed;
  a.waits = P.dag_waits;
  a.counters = P.dag_counters;
  a.n_tiles = (int)P.n_tiles;
  a.n_tasks = (int)P.n_dag_tasks;
  a.part = P.upd_part;
  a.split_cnt = P.upd_cnt;
  a.flag = flag;
  a.t_begin = t_begin;
  a.t_end = t_end;
  a.ticket = extra + (phase == 1 ? kDagOffTicket1 : kDagOffTicket0);
  a.progress = progress;
  a.trace = trace;
  a.first_store = (int)std::min<long>(first_store, INT_MAX);
  a.started = extra + (phase == 1 ? kDagOffStarted1 : kDagOffStarted0);
  a.wg_limit = g_dag_wg_limit;
  // A small task graph runs on fewer workgroups (a quarter of its tasks, at
  // least 64): its time is the elimination tree's chain, which runs faster
  // beside fewer co-resident update workgroups (cfg2, 580 tasks: 219.6 us on
  // 128 workgroups against 228.4 on 448; the incremental cfg2 flow's
  // minimizer 1.83 -> 1.79 ms per Solve).  cfg3 (12,625 tasks) keeps the full grid.
  const long ntk = t_end - t_begin;
  // (n_workgroups: at most the resident count, kDagWorkgroupsPerCu per CU --
  // the claim cap, half the grid, must leave resident workgroups free to draw;
  // DESIGN §8b.  The callers clamp it: a HIP query here would sit on the hot path)
  const int grid = dag_launch_grid(ntk, n_workgroups);
  hipLaunchKernelGGL(k_factor_dag, dim3((unsigned)grid), dim3(256), 0, s, a);
}

void launch_dense_back_solve_dag(const LltPlan &P, const double *S, long nR, double *yF, int *flag,
                                 hipStream_t s, int n_workgroups, bool reset) {
  const int ncols = (int)P.h_bcols.size();
  if (ncols == 0) return;
  if (reset) {
    (void)hipMemsetAsync(P.bs_counters, 0, ((size_t)P.T + 1) * sizeof(int), s);
    // y to the "not solved" pattern (both 32-bit halves of kYSentinel are equal)
    static_assert((kYSentinel >> 32) == (kYSentinel & 0xffffffffull), "kYSentinel halves");
    if (nR > 0) (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(yF), (int)(kYSentinel & 0xffffffffull),
                                        2 * (size_t)nR, s);
  }
  const int grid = std::min(n_workgroups, ncols);
  hipLaunchKernelGGL(k_bsolve_dag, dim3((unsigned)grid), dim3(256), 0, s, S, P.tile_id, P.T, P.ldiag, nR, P.bs_cols,
                     P.bs_gather, P.bs_gtile, P.bs_gbeg, ncols, yF, P.bs_counters, flag);
}

}  // namespace arslam
