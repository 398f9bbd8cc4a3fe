// llt_plan.h -- the reduced-system Cholesky as its users see it: the tile plan
// (`LltPlan`, built on the host by llt_plan.cpp), the counters, records and
// debug words of k_factor_dag's protocol, the host-side checks of the task
// graph, and the launchers of the two executors (llt_levels.hip, llt_dag.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "host_structure.h"

namespace arslam {
constexpr int kCuFlags = 2048;   // k_factor_dag's per-CU flags: 8 XCCs x 256 (SE, SH, CU) ids
// dag_counters after ready[n_tiles] | applied[n_tiles] (offsets from
// 2 n_tiles): the phase-0 ticket, the claimed-continuation count, the per-CU
// flags, the phase-1 ticket, and the fault record of a timed-out wait
// (kDagFault*: written once, by the workgroup whose fault code won the flag)
constexpr int kDagOffTicket0 = 0;
constexpr int kDagOffInflight = 1;
constexpr int kDagOffCuFlags = 2;
constexpr int kDagOffTicket1 = 2 + kCuFlags;
constexpr int kDagOffFault = 3 + kCuFlags;
enum DagFaultField {
  kFaultTicket = 0,   // the stuck ticket
  kFaultKind = 1,     // 1 dependency (early) wait, 2 in-order application, 3 late wait
  kFaultCounter = 2,  // the awaited counter: ready[c] (c < n_tiles) or applied[c - n_tiles]
  kFaultSeen = 3,     // its value when the wait gave up
  kFaultNeed = 4,     // the value it waited for
  kFaultDrawn = 5,    // tickets drawn by then (the launch's ticket counter)
  kFaultInflight = 6, // claimed continuations in flight
  kFaultBlock = 7,    // the workgroup
  kFaultFirstStuck = 8,   // INT_MAX - the smallest ticket whose wait ran out of time (0: none)
  kDagFaultSlots = 9
};
// workgroups of the phase-0 / phase-1 launch that have started (k_factor_dag's
// claim cap is half of these, not half the grid: DESIGN §8b)
constexpr int kDagOffStarted0 = kDagOffFault + kDagFaultSlots;
constexpr int kDagOffStarted1 = kDagOffStarted0 + 1;
constexpr int kDagCounterExtra = kDagOffStarted1 + 1;
// k_factor_dag workgroups resident per CU (its launch bounds; 73 KB of LDS
// each): a launch never asks for more than this times the CU count
constexpr int kDagWorkgroupsPerCu = 2;

// Fields of a ticket's record (LltPlan::dag_rec, 32 ints).  -1 where absent.
enum DagRecField {
  kRecType = 0, kRecY, kRecZ, kRecW,           // the task (type, y, z, w)
  kRecSub, kRecLate, kRecWait0, kRecWait1,     // fused TRSM tile, start of the late waits, the wait list
  kRecCont, kRecContAkk, kRecMaxdep,           // continuation target, its A_kk tile, own maxdep
  kRecContMaxdep, kRecContWait0, kRecContLate, // the target's maxdep and early-wait range
  kRecInv,                                     // POTRF: 1 if the task also inverts L_kk (the root column: no INV task)
  kRecQ0 = 16, kRecQ1,                         // POTRF fold / update item: columns [q0, q1) of ks
  kRecFoldK0, kRecFoldTile0,                   // POTRF: ks[q0] and tid(k, ks[q0])
  kRecSid = 18, kRecTi, kRecTj,                // update item: split slot, target tile (ti, tj)
  kRecSplitN, kRecSplitP,                      // update item of a split target: pieces, first partial slot
  kRecTile0I, kRecTile0J,                      // update item: its first column's operand tile ids
  kDagRecInts = 32
};

// k_factor_dag's debug outputs.  A ticket's trace words (launch_dense_llt_dag's trace, [n_tasks][kDagTraceWords],
// s_memrealtime ticks of 10 ns) -- tools/dag_trace.py, dag_phases.py and dag_critical.py read the dumped file by
// these numbers, so a change here is a change there:
enum DagTraceWord {
  kTrDraw = 0,           // the ticket was drawn (or its claimed run began)
  kTrMet = 1,            // its early waits were met
  kTrEnd = 2,            // the task ended
  kTrWg = 3,             // the workgroup; above bit 32 a POTRF with a fused tile adds 1 premet, 2 A_kk came in D,
                         // 4 fused tile prefetched, 8 the continuation's early waits seen met, 16 continuation claimed
  kTrLoaded = 4,         // POTRF: A_kk loaded and folded; TRSM: operands loaded
  kTrFactored = 5,       // POTRF: factorized; TRSM: solved
  kTrPublished = 6,      // POTRF: L_kk published
  kTrSubPublished = 7,   // POTRF: the fused tile published (0: none)
  // POTRF with a fused tile, the stretch between the two publishes (tools/potrf_cont.py; the trace file keeps
  // these four words in a block of their own behind the others, [n_tasks][kDagTraceSubWords]):
  kTrSolveTop = 8,       // the fused tile is in X and every wave is at the solve (the barrier before it)
  kTrWantKnown = 9,      // the claim's ticket count, started count and reservation are in hand
  kTrSolved = 10,        // every wave's solve steps are done (the barrier after them)
  kTrAcked = 11,         // the solved tile's stores are acknowledged (the barrier before its publish)
#ifdef ARSLAM_DAG_SUBSTAMPS
  // a stamped build only (the default library's trace keeps 12 words and its kernel its addressing): the waves'
  // own stamps inside the POTRF, blocked_potrf64_async's PfStamp words in their order -- wave 0 before and after
  // each of its three round waits, wave 0 at the closing barrier, waves 1-3 back from the last panel's side work
  kTrPfStamp0 = 12,      // .. + 9
  kDagTraceWords = 22
#else
  kDagTraceWords = 12
#endif
};
constexpr int kDagTraceFileWords = 8;   // the words of a ticket in the trace file's main block
constexpr int kDagTraceSubWords = kDagTraceWords - kDagTraceFileWords;
// and a workgroup's host-visible progress ints (launch_dense_llt_dag's progress, [grid][kDagProgressInts]):
enum DagProgressSlot {
  kProgTicket = 0,   // the ticket in hand
  kProgPhase = 1,    // 1 drawn, 2 waits met, 3 update item's products done, 4 task done, 9 left the loop
  kProgType = 2,     // its task type (kRecType)
  kDagProgressInts = 4
};

// Tile plan of the reduced-system Cholesky (llt_levels.hip, llt_dag.hip), level-scheduled
// over the tile elimination tree.  Device arrays, host per-level offsets.
struct LltPlan {
  // every device array of the plan lives in one grow-only arena (one
  // allocation and one host->device copy per load; kept across re-plans)
  char *arena = nullptr;
  size_t arena_bytes = 0;
  int T = 0;
  long lda = 0;
  int nlev = 0;
  int2 *panel = nullptr;        // (i,k) factor tasks; i == k is the diagonal tile
  int2 *upd_targets = nullptr;  // (i,j) tiles updated by a level
  int *upd_kstart = nullptr;    // CSR over targets of the contributing columns k
  int *upd_ks = nullptr;
  // work items of the update launches: {target, q0, q1, split} -- a target with
  // a long k-list is split into chunks whose partial products go to upd_part
  // and are summed in chunk order by the last-arriving chunk (deterministic)
  int4 *upd_items = nullptr;
  int2 *upd_split = nullptr;    // [n_split] {n_chunks, first partial slot}
  int *upd_cnt = nullptr;       // [n_split] arrival counters (zeroed per factorization)
  double *upd_part = nullptr;   // [n_part * 4096]
  long n_split = 0, n_part = 0;
  std::vector<int> h_item_off;      // [nlev+1]
  int *bs_cols = nullptr;       // backward-solve columns, root level first
  int2 *bs_gather = nullptr;    // (i,k) tiles gathered by each backward level, root level first
  int *bs_gbeg = nullptr;       // [ncols+1] gather range of each backward column (bs_cols order)
  int *bs_gtile = nullptr;      // [n_gather] tile_id of bs_gather's (i,k): k_bsolve_dag reads it, not the map
  double *bs_part = nullptr;    // [n_gather*64] per-gather partial sums L_ik^T y_i (summed in order)
  int *bs_counters = nullptr;   // [T+1] persistent backward solve: done[column] | ticket
  int *tile_id = nullptr;       // [T*T] compact index of tile (i,j), -1 if structurally zero
  std::vector<int> h_tile_id;
  long n_tiles = 0;             // tiles of the factor (compact storage = n_tiles * 4096 doubles)
  long n_assembled = 0;         // tiles the Schur assembly writes (numbered first; multi-rank: = n_top_tiles)
  bool fill_first_ok = false;   // every fill tile's first application is an unfolded update item (dag_build)
  // multi-rank plans (llt_plan_symbolic with column classes): phase 0 factors
  // this rank's subtree columns, phase 1 the replicated top columns after the
  // exchange of the top tiles (numbered first: tiles [0, n_top_tiles))
  int n_phases = 1;
  long phase_split = 0;         // tickets [0, phase_split) are phase 0
  long n_top_tiles = 0;
  std::vector<int> h_col_class; // [T] 0 own subtree, 1 top, 2 another rank's (not stored)
  std::vector<int> h_dag_phase; // [n_dag_tasks]
  signed char *tile_class = nullptr;   // [T] device copy of h_col_class
  double *ldiag = nullptr;      // 2T x 64 x 64: diagonal factors L_kk, then their inverses (row-major)
  std::vector<int> h_panel_off;     // [nlev+1]
  std::vector<int> h_upd_off;       // [nlev+1]
  std::vector<int> h_bs_off;        // [nlev+1], in backward (root-first) order
  std::vector<int> h_bsg_off;       // [nlev+1], gather tasks per backward level
  std::vector<double> h_upd_flops;  // useful flops of each level's update
  // persistent task-graph executor (launch_dense_llt_dag), host side: tasks
  // in ticket order {type, a, b, c} (0 POTRF k; 1 TRSM i,k; 2 update item a,
  // level sequence b, target tile c), each with a list of {counter, value}
  // waits (h_dag_wait_off); counters = [ready(n_tiles) | applied(n_tiles) |
  // ticket].  h_dag_sub[t] = {tile id of the TRSM fused into POTRF task t or
  // -1, index in the waits where that TRSM's late waits begin}.
  // h_dag_cont[t]: the POTRF task the workgroup finishing POTRF task t may run
  // next (the parent column, whose fold is exactly the tile t solved) or -1;
  // h_dag_maxdep[t]: for such targets the largest ticket t waits on, else -1;
  // h_dag_cont_akk[t]: the storage index of the target's A_kk when the target
  // folds task t's column alone (its A_kk is then all it loads, and task t's
  // workgroup prefetches it beside the fused solve), else -1.
  // dag_claimed[t] (device): taken by the predecessor's workgroup or by the drawer.
  std::vector<int2> h_dag_sub;
  int *dag_claimed = nullptr;
  std::vector<int> h_dag_cont, h_dag_maxdep, h_dag_cont_akk;
  // the column whose POTRF task also computes L_kk^{-1} (kRecInv) and that has
  // no INV task: the last tile column when it ends the last phase, else -1
  int root_inv_col = -1;
  // dag_rec[32 t ..]: every field the executor reads about ticket t, in one
  // 128-byte record (kDagRec* offsets), fetched with two scalar loads -- the
  // separate arrays were a chain of dependent loads (task -> item -> column
  // -> tile id), each a memory round trip under the factorization's traffic.
  // dag_ks_tiles[q]: the operand tile ids {tid(ti, ks[q]), tid(tj, ks[q])} of
  // column q of an update item with target (ti, tj).
  int *dag_rec = nullptr;
  int2 *dag_ks_tiles = nullptr;
  std::vector<int> h_dag_rec;
  std::vector<int2> h_dag_ks_tiles;
  // (dag_counters = [ready | applied | ticket | inflight | kCuFlags per-CU flags | phase-1 ticket |
  //  fault record], kDagOff*)
  int2 *dag_waits = nullptr;
  int *dag_counters = nullptr;
  long n_dag_tasks = 0;
  std::vector<int4> h_dag_tasks;
  std::vector<int> h_dag_wait_off;
  std::vector<int2> h_dag_waits;
  // host copies of the device lists (llt_plan_symbolic)
  std::vector<int2> h_panel, h_targets, h_gather, h_split;
  std::vector<int> h_kstart, h_ks, h_bcols, h_gbeg, h_gtile;
  std::vector<int4> h_items;
  double total_upd_flops = 0.0;
  double total_factor_flops = 0.0;   // updates + POTRF (+ inverse) + TRSM of the task graph
  long total_upd_tiles = 0;
};

// Symbolic tile fill of the lower pattern (T*T bytes, in/out) and the host
// task lists (no HIP calls: usable without a device).
// (col_class: null = one rank; else per tile column 0 this rank's subtree,
// 1 the replicated top, 2 another rank's -- a two-phase plan, see LltPlan)
void llt_plan_symbolic(LltPlan &plan, int T, long lda, std::vector<uint8_t> &pattern,
                       const std::vector<int> *col_class = nullptr);
// Subtree-to-rank split of the tile elimination tree (multi-GPU): the top of
// the tree (the upper nested-dissection separators, the camera and the rhs)
// is replicated, the subtrees below it are dealt to the ranks, and every
// capture goes to the rank owning the lowest tile column of its tags (its
// columns lie on one root path: they are pairwise coupled), or, if its tags
// are all in the top, to the rank with the fewest observations so far.
struct RankSplit {
  std::vector<int> col_owner;   // [T] owning rank, -1 = top (replicated)
  std::vector<int> cap_owner;   // [nc]
  int n_top_cols = 0;
  int n_active = 0;             // ranks owning subtrees (the others own top-only captures)
  double top_work = 0.0, max_rank_work = 0.0, total_work = 0.0;   // tile-task counts
  std::vector<int> col_class(int rank) const {   // llt_plan_symbolic's classes
    std::vector<int> c(col_owner.size());
    for (size_t k = 0; k < c.size(); ++k) c[k] = col_owner[k] < 0 ? 1 : (col_owner[k] == rank ? 0 : 2);
    return c;
  }
};
RankSplit rank_split(const HostProblem &h, const ReducedLayout &L, int nranks);
// Ticket-order check of the task graph: executing the tasks one at a time in
// ticket order, is every wait already satisfied when its task runs?
bool dag_check(const LltPlan &plan);
// Randomised (policy 0) or adversarial interleavings of n_workers workgroups
// running k_factor_dag's protocol; false on a reachable deadlock (dag_simulate
// in llt_plan.cpp lists the policies).
// n_started >= 0: only that many of the n_workers workgroups ever start, one
// at a time as the schedule picks them (fewer resident than the grid).
bool dag_simulate(const LltPlan &plan, int n_workers, unsigned seed, int policy = 0, int n_started = -1);
constexpr int kDagSimPolicies = 4;
constexpr int kDagSimNoCap = 16;
constexpr int kDagSimGridCap = 32;   // (tests) round 5's cap: half the grid, not half the started workgroups
// dag_simulate over small grids, the executor's own and 512, every policy, and
// grids of which only a few workgroups start: 1 if deadlock-free in every run,
// else -(grid * 16 + policy) of the first deadlock (-100000 k more when only k started).
int dag_simulate_all(const LltPlan &plan);
// The fault record of a timed-out executor wait (kDagFault*) in words: the
// stuck task, the awaited counter, its producers and how far the launch drew.
std::string dag_fault_detail(const LltPlan &plan, const int *rec);
// Upload the host lists and allocate the plan's device buffers.
void llt_plan_upload(LltPlan &plan, hipStream_t s);
// llt_plan_symbolic + llt_plan_upload
void llt_plan_build(LltPlan &plan, int T, long lda, std::vector<uint8_t> &pattern, hipStream_t s,
                    const std::vector<int> *col_class = nullptr);
void llt_plan_free(LltPlan &plan);                 // device arrays and the arena
void llt_plan_reset(LltPlan &plan);                // host side only; the arena is kept for the next plan

// Optional per-launch event pairs around the dominant kernel (trailing update).
struct LaunchTiming {
  hipEvent_t *ev = nullptr;   // 2 * cap events
  int cap = 0;
  int used = 0;
  double flops = 0.0;         // algorithmic flops of the recorded launches
};

// ---- llt_levels.hip (launch_dense_llt, launch_dense_back_solve), llt_dag.hip (the rest) ----
// Cholesky of the lower triangle of S (row-major, lda) over the plan's tiles,
// in place.  Row nR carries the right-hand side, so on exit row nR =
// (L^{-1} b)^T.  *flag is set non-zero if a pivot is not positive.
void launch_dense_llt(const LltPlan &P, double *S, int *flag, hipStream_t s,
                      LaunchTiming *timing = nullptr);
// Then y = L^{-T} z into yF[0..nR).
void launch_dense_back_solve(const LltPlan &P, const double *S, long nR, double *z, double *yF,
                             const int *flag, hipStream_t s);
// debug: only the first k workgroups of every k_factor_dag launch start (the
// others return at once; k <= 0 restores all), process-wide
void set_dag_workgroup_limit(int k);
// k_factor_dag's grid for n_tasks tickets when n_workgroups are asked for: a small task graph
// runs on fewer workgroups (a quarter of its tasks, at least 64; launch_dense_llt_dag)
inline int dag_launch_grid(long n_tasks, int n_workgroups) {
  return (int)std::min<long>(n_workgroups, std::max<long>(std::min<long>(64, n_tasks), n_tasks / 4));
}
// The same factorization as launch_dense_llt's as one persistent launch over
// the plan's task graph (tickets in a topological order, dependency counters
// in global memory).
// (reset = false: the counters were zeroed by launch_exec_reset)
// (phase: -1 every task; 0 / 1 one phase of a multi-rank plan, LltPlan)
// (first_store: the tiles from first_store on are fill tiles the Schur gather
// does not write and S is not cleared for -- their first update stores
// instead of reading the tile; LONG_MAX: none)
void launch_dense_llt_dag(const LltPlan &P, double *S, int *flag, hipStream_t s, int n_workgroups,
                          int *progress = nullptr, unsigned long long *trace = nullptr, bool reset = true,
                          int phase = -1, long first_store = LONG_MAX);
// The same backward solve as one persistent launch (columns in root-first
// ticket order, per-column completion counters).
void launch_dense_back_solve_dag(const LltPlan &P, const double *S, long nR, double *yF, int *flag,
                                 hipStream_t s, int n_workgroups, bool reset = true);
// k_bsolve_dag's "not solved yet" value of a y entry: a signalling-NaN bit
// pattern no arithmetic produces (those NaNs are quiet)
constexpr unsigned long long kYSentinel = 0x7ff47ff47ff47ff4ull;
// the LM diagonal clamp(s^2 colnorm, dmin, dmax) over n slots (k_lm_diag): work
// the executors' reset launch, and the LM launches of lm_launch.h, can carry
struct LmDiagArgs {
  long n;
  const double *scale, *colnorm;
  double dmin, dmax;
  double *diag;
  double *ysent = nullptr;   // (also: the backward solve's y, nys rows, to kYSentinel)
  long nys = 0;
};
// *flag and every counter of the two persistent executors to zero, one launch
// (with ld: the LM diagonal in the same launch)
void launch_exec_reset(const LltPlan &P, int *flag, hipStream_t s, const LmDiagArgs *ld = nullptr);
// The same reset as element-wise work another launch can carry (k_schur's
// blocks past the captures and tiles, when the diagonal needs no update):
// element e < n() zeroes one counter / writes one y sentinel; e == 0 also the flag.
struct ExecReset {
  int *flag = nullptr;
  int *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
  long na = 0, nb = 0, nc = 0, nd = 0;
  double *ysent = nullptr;
  long nys = 0;
  __host__ __device__ long n() const { return na + nb + nc + nd > nys ? na + nb + nc + nd : nys; }
};
ExecReset exec_reset_args(const LltPlan &P, int *flag, double *ysent, long nys);
__device__ __forceinline__ void exec_reset_elem(const ExecReset &r, long e) {
  if (e < r.nys) r.ysent[e] = __longlong_as_double((long long)kYSentinel);
  if (e < r.na) r.a[e] = 0;
  else if (e < r.na + r.nb) r.b[e - r.na] = 0;
  else if (e < r.na + r.nb + r.nc) r.c[e - r.na - r.nb] = 0;
  else if (e < r.na + r.nb + r.nc + r.nd) r.d[e - r.na - r.nb - r.nc] = 0;
  if (e == 0 && r.flag) *r.flag = 0;
}
void launch_zero_tiles(const LltPlan &P, double *S, hipStream_t s);
// copy the diagonal factors L_kk into S (tests only: S then holds the whole factor)
void launch_scatter_diag(const LltPlan &P, double *S, hipStream_t s);

}  // namespace arslam
