// debug_plans.cpp -- host-only component entry points (include/arslam_lm_debug.h):
// what a load derives from a problem before any device call -- the reduced
// layout, the symbolic tile plan and its task graph, the rank split, Ceres'
// e-block set, the Schur gather plan and k_schur's store table -- so the CPU
// tests can probe it without a device.
#include "llt_plan.h"
#include "lm_launch.h"
#include "lm_problem.h"
#include "schur_store_table.h"
#include "arslam_lm.h"
#include "arslam_lm_debug.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
using namespace arslam;

// What a one-rank load derives on the host: the problem's structure, the reduced system's
// layout (nested dissection, zero tiles skipped, unless asked otherwise) and its symbolic plan.
struct HostPlan {
  HostProblem h;
  ReducedLayout L;
  LltPlan plan;   // (symbolic())
  explicit HostPlan(HostProblem hp, const LayoutRequest &rq = {}) : h(std::move(hp)), L(reduced_layout(h, rq)) {}
  explicit HostPlan(const arslam_soa_problem *p) : HostPlan(host_problem(p)) {}
  bool reduced() const { return L.nR > 0; }
  // cls: a rank's column classes (RankSplit::col_class), null = the one-phase plan
  HostPlan &symbolic(const std::vector<int> *cls = nullptr) {
    api_check(reduced(), ARSLAM_E_INVALID_ARG, "no reduced system");
    llt_plan_symbolic(plan, L.T, L.N, L.pattern, cls);
    return *this;
  }
};

// (dag_valid: the ticket-order check only; the callers that simulate overwrite it)
void fill_plan_info(const HostPlan &hp, arslam_plan_info *info) {
  const ReducedLayout &L = hp.L;
  const LltPlan &plan = hp.plan;
  std::memset(info, 0, sizeof(*info));
  info->n_reduced = L.nR;
  info->n_padded = L.N;
  info->pad_rows = L.pad_rows;
  info->tiles_per_side = L.T;
  info->n_parts = L.n_parts;
  info->camera_row = L.cam_row;
  info->scalar_flops = L.scalar_flops;
  if (!hp.reduced()) return;   // (else after symbolic())
  info->n_levels = plan.nlev;
  info->n_assembled_tiles = plan.n_assembled;
  info->n_factor_tiles = plan.n_tiles;
  info->n_update_tiles = plan.total_upd_tiles;
  info->n_update_items = (long)plan.h_items.size();
  info->n_split_targets = (long)plan.h_split.size();
  info->update_flops = plan.total_upd_flops;
  info->factor_flops = plan.total_factor_flops;
  info->n_dag_tasks = plan.n_dag_tasks;
  info->fill_first_ok = plan.fill_first_ok ? 1 : 0;
  info->dag_valid = dag_check(plan) ? 1 : 0;
}

// ARSLAM_DAG_DUMP: the task graph, for offline analysis (tools/dag_dump.py reads it)
void dump_dag(const LltPlan &plan, const char *path) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return;
  const long n = plan.n_dag_tasks, nw = (long)plan.h_dag_waits.size(), T = plan.T;
  std::fwrite(&n, 8, 1, f);
  std::fwrite(&nw, 8, 1, f);
  std::fwrite(&T, 8, 1, f);
  const long ni = (long)plan.h_items.size(), ntg = (long)plan.h_targets.size();
  std::fwrite(&ni, 8, 1, f);
  std::fwrite(&ntg, 8, 1, f);
  std::fwrite(plan.h_dag_tasks.data(), sizeof(int4), n, f);
  std::fwrite(plan.h_dag_wait_off.data(), sizeof(int), n + 1, f);
  std::fwrite(plan.h_dag_waits.data(), sizeof(int2), nw, f);
  std::fwrite(plan.h_dag_sub.data(), sizeof(int2), n, f);
  std::fwrite(plan.h_tile_id.data(), sizeof(int), (size_t)T * T, f);
  std::fwrite(plan.h_items.data(), sizeof(int4), plan.h_items.size(), f);
  std::fwrite(plan.h_targets.data(), sizeof(int2), plan.h_targets.size(), f);
  std::fwrite(plan.h_dag_cont.data(), sizeof(int), n, f);
  std::fwrite(plan.h_dag_maxdep.data(), sizeof(int), n, f);
  // the backward solve's gather list: {i, k} and the stored tile index of each entry
  const long ng = (long)plan.h_gather.size();
  std::fwrite(&ng, 8, 1, f);
  std::fwrite(plan.h_gather.data(), sizeof(int2), ng, f);
  std::fwrite(plan.h_gtile.data(), sizeof(int), ng, f);
  std::fclose(f);
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

extern "C" int arslam_debug_reduced_plan(const arslam_soa_problem *p, int ordering, int skip_zero_tiles,
                                         arslam_plan_info *info, int *tag_row) {
  if (!p || !info || ordering < 0 || ordering > 2) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    std::memset(info, 0, sizeof(*info));
    static const bool prof = std::getenv("ARSLAM_SETUP_PROFILE") != nullptr;   // debug: setup phases
    const double t0 = now_ms();
    HostProblem h = host_problem(p);
    const double t1 = now_ms();
    LayoutRequest rq;
    rq.ordering = ordering;
    rq.sparse = skip_zero_tiles != 0;
    HostPlan hp(std::move(h), rq);
    const double t2 = now_ms();
    if (tag_row)
      for (int t = 0; t < hp.h.nt; ++t) tag_row[t] = hp.L.tag_row[t];
    if (hp.reduced()) {
      hp.symbolic();
      if (prof) std::fprintf(stderr, "arslam plan: host_problem %.3f layout %.3f plan %.3f ms\n", t1 - t0, t2 - t1, now_ms() - t2);
    }
    fill_plan_info(hp, info);
    if (!hp.reduced()) return;
    if (const char *dump = std::getenv("ARSLAM_DAG_DUMP")) dump_dag(hp.plan, dump);
    if (info->dag_valid) info->dag_valid = dag_simulate_all(hp.plan);
  });
}

// The side a one-rank load eliminates when asked for `elimination` (CAPTURES, TAGS or MIXED: Ceres' set e_cap /
// e_tag, or a whole side where the set holds one kind only -- arslam_lm::choose_side's rule).
static int debug_side(const arslam_soa_problem *p, int elimination, std::vector<uint8_t> &e_cap,
                      std::vector<uint8_t> &e_tag) {
  if (elimination != ARSLAM_ELIM_MIXED) return elimination;
  const SchurSide cs = ceres_schur_side(p, &e_cap, &e_tag);
  if (cs.e_cam || cs.e_tag == 0) return ARSLAM_ELIM_CAPTURES;
  return cs.e_cap == 0 ? ARSLAM_ELIM_TAGS : ARSLAM_ELIM_MIXED;
}

extern "C" int arslam_debug_reduced_plan_side(const arslam_soa_problem *p, int elimination, arslam_plan_info *info) {
  if (!p || !info || elimination < ARSLAM_ELIM_CAPTURES || elimination > ARSLAM_ELIM_MIXED) return ARSLAM_E_INVALID_ARG;
  int side = elimination;
  const int rc = api_guarded([&] {
    std::memset(info, 0, sizeof(*info));
    // the device problem of that side, as arslam_lm's load builds it (one rank)
    std::vector<uint8_t> e_cap, e_tag;
    MixedProblem mx;
    arslam_soa_problem swapped;
    side = debug_side(p, elimination, e_cap, e_tag);
    const arslam_soa_problem *q = device_problem(*p, side, e_cap, e_tag, swapped, mx);
    HostPlan hp(device_host_problem(q, side == ARSLAM_ELIM_MIXED ? &mx : nullptr, *p));
    if (hp.reduced()) hp.symbolic();
    fill_plan_info(hp, info);
  });
  return rc ? rc : side;
}

extern "C" int arslam_debug_order_memory(const arslam_soa_problem *problems, int n_problems, int elimination,
                                         int ordering, const unsigned char *forget_before, arslam_order_step *steps,
                                         int *const *tag_row, int *const *cap_row) {
  if (!problems || !steps || n_problems < 1 || elimination < ARSLAM_ELIM_CAPTURES || elimination > ARSLAM_ELIM_MIXED ||
      ordering < 0 || ordering > 2)
    return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    OrderMemory order;
    for (int i = 0; i < n_problems; ++i) {
      const arslam_soa_problem &p = problems[i];
      if (forget_before && forget_before[i]) order.forget();
      // load()'s one-rank stages up to the remembered order, the first as a
      // first load, the later ones as the pointer-keyed path's reloads
      const bool reuse = i > 0;
      std::vector<uint8_t> e_cap, e_tag;
      MixedProblem mx;
      arslam_soa_problem swapped;
      const int side = debug_side(&p, elimination, e_cap, e_tag);
      const arslam_soa_problem *q = device_problem(p, side, e_cap, e_tag, swapped, mx);
      const MixedProblem *mixed = side == ARSLAM_ELIM_MIXED ? &mx : nullptr;
      LayoutRequest rq = order.request(reuse, side, mixed, ordering, true, q->n_cap);
      const HostProblem h = device_host_problem(q, mixed, p);
      rq.fast_order = reuse;
      bool recomputed = false;
      const ReducedLayout L = order.layout(h, rq, &recomputed);
      order.remember(L, h, rq, mixed);
      steps[i] = {side, L.order_reused ? 1 : 0, recomputed ? 1 : 0, L.nR > 0 ? etree_height(L) : 0, L.pad_rows};
      // the rows by the caller's blocks
      int *tr = tag_row ? tag_row[i] : nullptr, *cr = cap_row ? cap_row[i] : nullptr;
      if (tr) std::fill(tr, tr + p.n_tag, -1);
      if (cr) std::fill(cr, cr + p.n_cap, -1);
      for (int f = 0; f < h.nt; ++f) {
        const bool is_cap = mixed ? mx.f_is_cap[f] != 0 : side == ARSLAM_ELIM_TAGS;
        int *out = is_cap ? cr : tr;
        if (out) out[mixed ? mx.f_src[f] : f] = L.tag_row[f];
      }
    }
  });
}

extern "C" int arslam_debug_dag_simulate(const arslam_soa_problem *p, int n_workers, unsigned seed, int policy,
                                         int *ok) {
  if (!p || !ok || n_workers < 1 || policy < 0) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] { *ok = dag_simulate(HostPlan(p).symbolic().plan, n_workers, seed, policy) ? 1 : 0; });
}

extern "C" int arslam_debug_dag_simulate_started(const arslam_soa_problem *p, int n_workers, int n_started,
                                                 unsigned seed, int policy, int *ok) {
  if (!p || !ok || n_workers < 1 || n_started < 0 || policy < 0) return ARSLAM_E_INVALID_ARG;
  return api_guarded(
      [&] { *ok = dag_simulate(HostPlan(p).symbolic().plan, n_workers, seed, policy, n_started) ? 1 : 0; });
}

extern "C" int arslam_debug_dag_workgroup_limit(int k) {
  set_dag_workgroup_limit(k);
  return ARSLAM_OK;
}

extern "C" int arslam_debug_dag_fault_detail(const arslam_soa_problem *p, const int rec[9], char *buf, int len) {
  if (!p || !rec || !buf || len <= 0) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    const std::string s = dag_fault_detail(HostPlan(p).symbolic().plan, rec);
    std::snprintf(buf, (size_t)len, "%s", s.c_str());
  });
}

extern "C" int arslam_debug_rank_split(const arslam_soa_problem *p, int nranks, int rank, arslam_split_info *info,
                                       int *cap_owner) {
  if (!p || !info || nranks < 1 || rank < 0 || rank >= nranks) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    std::memset(info, 0, sizeof(*info));
    HostPlan hp(p);
    const RankSplit split = rank_split(hp.h, hp.L, nranks);
    info->tiles_per_side = hp.L.T;
    info->top_work = split.top_work;
    info->max_rank_work = split.max_rank_work;
    info->total_work = split.total_work;
    info->n_active = split.n_active;
    for (int c = 0; c < hp.h.nc; ++c) {
      if (cap_owner) cap_owner[c] = split.cap_owner[c];
      info->n_owned_captures += split.cap_owner[c] == rank;
    }
    if (!hp.reduced()) return;
    const std::vector<int> cls = split.col_class(rank);
    for (int k = 0; k < hp.L.T; ++k) {
      info->n_top_cols += cls[k] == 1;
      info->n_own_cols += cls[k] == 0;
    }
    const LltPlan &plan = hp.symbolic(nranks > 1 ? &cls : nullptr).plan;
    info->n_top_tiles = plan.n_top_tiles;
    info->n_tiles = plan.n_tiles;
    info->n_dag_tasks = plan.n_dag_tasks;
    info->phase_split = plan.phase_split;
    info->dag_valid = dag_check(plan) ? 1 : 0;
    if (info->dag_valid) info->dag_valid = dag_simulate_all(plan);
  });
}

// Host-only: the task graph of the plan the solver makes for `rank` of `nranks` (1: the one-rank plan), in ticket
// order: tasks[4 t ..] = {type, y, z, w} (LltPlan::h_dag_tasks) and phase[t], for the first `cap` tickets; *n_tasks
// the plan's count; info = {tile columns T, phase_split, n_phases, root_inv_col}.
extern "C" int arslam_debug_dag_tasks(const arslam_soa_problem *p, int nranks, int rank, int *tasks, int *phase,
                                      long cap, long *n_tasks, int info[4]) {
  if (!p || !n_tasks || !info || nranks < 1 || rank < 0 || rank >= nranks || cap < 0 || (cap > 0 && (!tasks || !phase)))
    return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    HostPlan hp(p);
    api_check(hp.reduced(), ARSLAM_E_INVALID_ARG, "no reduced system");
    std::vector<int> cls;
    if (nranks > 1) cls = rank_split(hp.h, hp.L, nranks).col_class(rank);
    const LltPlan &plan = hp.symbolic(nranks > 1 ? &cls : nullptr).plan;
    *n_tasks = plan.n_dag_tasks;
    for (long t = 0; t < std::min(cap, plan.n_dag_tasks); ++t) {
      const int4 k = plan.h_dag_tasks[t];
      tasks[4 * t] = k.x, tasks[4 * t + 1] = k.y, tasks[4 * t + 2] = k.z, tasks[4 * t + 3] = k.w;
      phase[t] = plan.h_dag_phase[t];
    }
    info[0] = plan.T, info[1] = (int)plan.phase_split, info[2] = plan.n_phases, info[3] = plan.root_inv_col;
  });
}

extern "C" int arslam_debug_ceres_e_blocks(const arslam_soa_problem *p, int out[4]) {
  if (!p || !out) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    const SchurSide cs = ceres_schur_side(p);
    out[0] = cs.e_cap;
    out[1] = cs.e_tag;
    out[2] = cs.e_cam;
    out[3] = cs.max_tag_obs;
  });
}

extern "C" int arslam_debug_mixed_groups(const arslam_soa_problem *p, int out[4], unsigned char *e_cap,
                                         unsigned char *e_tag) {
  if (!p || !out) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    std::vector<uint8_t> ec, et;
    (void)ceres_schur_side(p, &ec, &et);
    if (e_cap) std::copy(ec.begin(), ec.end(), e_cap);
    if (e_tag) std::copy(et.begin(), et.end(), e_tag);
    const MixedProblem m = mixed_problem(*p, ec, et);
    const HostProblem h = device_host_problem(&m.soa, &m, *p);
    out[0] = h.nc;
    out[1] = h.nt;
    out[2] = m.n_direct;
    out[3] = h.maxblk;
  });
}

// diagnostic build only (-DARSLAM_SCHUR_STAMPS): accumulated per-phase cycles of k_schur
extern "C" int arslam_debug_schur_stamps(unsigned long long out[16]) {
  if (!out) return ARSLAM_E_INVALID_ARG;
  debug_read_schur_stamps(out);
  return ARSLAM_OK;
}

// host only: k_schur<false>'s output-stage descriptors (the host copy of the table the kernel reads)
extern "C" int arslam_debug_schur_store_table(int nblk, int *off, unsigned char *stored) {
  static constexpr SchurStoreTable kTable = make_schur_store_table();
  if (!off || !stored || nblk < 1 || nblk > kSchurMfmaBlocks) {
    set_last_error("arslam_debug_schur_store_table: nblk outside 1..kSchurMfmaBlocks or a null array");
    return ARSLAM_E_INVALID_ARG;
  }
  const uint32_t *e = &kTable.e[nblk - 1][0][0][0];
  for (int s = 0; s < kSchurStoreTiles * kWave * 4; ++s) {
    off[s] = (int)((e[s] & kSchurStoreMask) >> 3);
    stored[s] = (e[s] >> 31) ? 0 : 1;
  }
  return ARSLAM_OK;
}

extern "C" int arslam_debug_gather_extend(const arslam_soa_problem *p, int c0, int *identical, int *n_dest) {
  if (!p || !identical || !n_dest || c0 < 0 || c0 > p->n_cap) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    // the first c0 captures' residual blocks, in p's order
    std::vector<int> oc, ot;
    std::vector<double> cr;
    for (int b = 0; b < p->n_obs; ++b)
      if (p->obs_cap[b] < c0) {
        oc.push_back(p->obs_cap[b]);
        ot.push_back(p->obs_tag[b]);
        cr.insert(cr.end(), p->corners + 8L * b, p->corners + 8L * b + 8);
      }
    arslam_soa_problem q = *p;
    q.n_cap = c0;
    q.n_obs = (int)oc.size();
    q.obs_cap = oc.data();
    q.obs_tag = ot.data();
    q.corners = cr.data();
    const HostPlan hs(&q);
    SchurGather G = schur_gather_plan(hs.h, hs.L);
    const HostProblem hf = host_problem(p);
    schur_gather_extend(G, hf, hs.L, c0);
    const SchurGather F = schur_gather_plan(hf, hs.L);
    bool same = G.cap_off == F.cap_off && G.dest_row == F.dest_row && G.dest_start == F.dest_start &&
                G.items == F.items && G.splits == F.splits && G.n_pslots == F.n_pslots &&
                G.max_contrib == F.max_contrib && G.contrib.size() == F.contrib.size();
    for (size_t i = 0; same && i < G.contrib.size(); ++i)
      same = !std::memcmp(&G.contrib[i], &F.contrib[i], sizeof(SchurContrib));
    *identical = same ? 1 : 0;
    *n_dest = (int)F.dest_start.size() - 1;
  });
}
