// lm_solve.hip -- the LM handle's solve (lm_handle.h): the trust-region loop,
// the stages of one step, the linearization and the write-back.
//
// The trust-region loop restates Ceres 2.0's TrustRegionMinimizer +
// LevenbergMarquardtStrategy as configured by ArSlamSolver::optimize
// (ar_slam_util.cpp:1001-1018).  Only scalars cross
// PCIe per step (cost, model cost change, norms, the Cholesky flag); the
// problem, the parameters and the reduced system stay resident in HBM.
#include "lm_handle.h"

// decode the persistent executors' negative flags (llt_dag.hip) ...
std::string arslam::lmh::executor_fault_message(int code, int rank, int iteration, const arslam::LltPlan &plan,
                                                hipStream_t s) {
  std::string what;
  const int c = -code;
  if (code == 0) what = "on another rank";
  else if (c >= 4000000) what = "backward-solve column " + std::to_string(c - 4000000) + ": dependency wait timed out";
  else if (c >= 3000000) what = "ticket " + std::to_string(c - 3000000) + ": late wait (fused TRSM / folded TRSM's L_kk) timed out";
  else if (c >= 2000000) what = "ticket " + std::to_string(c - 2000000) + ": in-order update wait timed out";
  else if (c >= 1000000) what = "ticket " + std::to_string(c - 1000000) + ": dependency wait timed out";
  else what = "code " + std::to_string(code);
  const std::string m = "reduced-system executor fault (rank " + std::to_string(rank) + ", LM iteration " +
                        std::to_string(iteration) + "): " + what;
  // ... and, for a timed-out wait of k_factor_dag, what its fault record says:
  // the awaited counter, the tickets that advance it, how far the launch drew
  // (read after the step's stream sync; the record is reset with the counters)
  if (code > -1000000 || code <= -4000000 || !plan.dag_counters) return m;
  int rec[arslam::kDagFaultSlots];
  if (hipMemcpyAsync(rec, plan.dag_counters + 2 * plan.n_tiles + arslam::kDagOffFault, sizeof(rec),
                     hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess || rec[arslam::kFaultTicket] != (-code) % 1000000)
    return m;
  return m + " -- " + arslam::dag_fault_detail(plan, rec);
}

void arslam_lm::timing_begin() {
  if (!opt.kernel_timing || !has_f) return;
  const int need = plan.nlev + 1;
  if ((int)upd_events.size() < 2 * need) {
    for (auto e : upd_events) (void)hipEventDestroy(e);
    upd_events.assign(2 * need, nullptr);
    for (auto &e : upd_events) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));   // (as Timer)
  }
  upd_timing.ev = upd_events.data();
  upd_timing.cap = need;
  upd_timing.used = 0;
  upd_timing.flops = 0.0;
}

void arslam_lm::timing_collect() {
  if (!opt.kernel_timing || !has_f) return;
  for (int i = 0; i < upd_timing.used; ++i) {
    float ms = 0.f;
    HIP_CHECK(hipEventSynchronize(upd_events[2 * i + 1]));
    HIP_CHECK(hipEventElapsedTime(&ms, upd_events[2 * i], upd_events[2 * i + 1]));
    dom_ms += ms;
  }
  dom_launches += upd_timing.used;
  dom_flops += upd_timing.flops;
  upd_timing.used = 0;
  upd_timing.flops = 0.0;
}

void arslam_lm::allreduce_any(void *buf, size_t count, int dtype, int op) {
  if (!multi() || count == 0) return;
  const size_t bytes = count * (dtype == ARSLAM_DT_F64 ? sizeof(double) : 1);
  comm_bytes += (double)bytes;
  ++comm_calls;
  if (comm_cb) {
    comm_stage.resize(bytes);
    HIP_CHECK(hipMemcpyAsync(comm_stage.data(), buf, bytes, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    fail_if(comm_cb(comm_cb_ctx, comm_stage.data(), count, dtype, op) != 0, ARSLAM_E_COMM,
            "all-reduce callback failed");
    HIP_CHECK(hipMemcpyAsync(buf, comm_stage.data(), bytes, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    return;
  }
  fail_if(!comm, ARSLAM_E_STATE, "the multi-rank path without a communicator");
  NCCL_CHECK(ncclAllReduce(buf, buf, count, dtype == ARSLAM_DT_F64 ? ncclDouble : ncclUint8,
                           op == ARSLAM_OP_SUM ? ncclSum : ncclMax, comm, stream));
}

// Evaluate residuals/Jacobian at x: cost, gradient (unscaled), column norms
// and the norms the minimizer reads.  Ceres EvaluateGradientAndJacobian.
void arslam_lm::linearize_launch() {
  h_lin.alloc(32);
  // one rank: the reductions also store their results straight into the
  // page-locked h_lin (no copy launch); several: h_lin is copied after the exchanges
  const bool direct = !multi();
  timers[PH_LIN].start(stream);
  arslam::launch_linearize(P, x, d_g.p, d_colnorm.p, d_obs_tg.p, d_parts.p, stream, cl());
  // (several ranks: this rank's partial cost and fixed cost also saved, the
  // step's reductions reuse d_red, for the scalar exchange; the LM diagonal
  // from the partial sums is final for the capture slots and this rank's own
  // subtree tags -- all their observations are this rank's -- the rest
  // follows the exchange, lin_norms)
  arslam::launch_lin_reduce(P, d_obs_tg.p, d_g.p, d_colnorm.p, d_parts.p, d_red.p, stream,
                            direct ? h_lin.p : nullptr, multi() ? d_red.p + kLinSave : nullptr);
  if (multi()) lin_xpending = true;
  const arslam::LmDiagArgs ld{n, d_scale.p, d_colnorm.p, opt.min_lm_diagonal, opt.max_lm_diagonal, d_diag.p};
  lin_seq = direct ? next_seq(h_lin.p + 16 + arslam::kHostSeq) : 0.0;
  // (l1, l2 estimated: their gradient and column norms from d_lparts first)
  arslam::launch_slot_norms(P, d_red.p, d_g.p, d_colnorm.p, x, d_norms_p, stream, direct ? h_lin.p + 16 : nullptr,
                            diag_in_lin ? &ld : nullptr, lin_seq, cl());
  timers[PH_LIN].stop(stream);
}

// (several ranks) the norms and the LM diagonal again, from the exchanged sums
void arslam_lm::lin_norms() {
  const arslam::LmDiagArgs ld{n, d_scale.p, d_colnorm.p, opt.min_lm_diagonal, opt.max_lm_diagonal, d_diag.p};
  arslam::launch_slot_norms(P, d_red.p, d_g.p, d_colnorm.p, x, d_norms_p, stream, nullptr, diag_in_lin ? &ld : nullptr,
                            0.0, cl());
  lin_xpending = false;
  norms_pending = true;   // capture slots and the held f-side slots: combined with the next scalars
}

// (several ranks) a pending linearization's sums when no step carries them:
// every tag slot's gradient and column norm and the camera's f partials, one
// packed all-reduce (the tags' observations span the ranks)
void arslam_lm::complete_pending_lin() {
  if (!lin_xpending) return;
  const long t0 = 3 + 6L * nc;
  arslam::PackSegs sg;
  sg.add(d_g.p + t0, n - t0);
  sg.add(d_colnorm.p + t0, n - t0);
  sg.add(d_red.p + arslam::P_GF, 2);   // g_f, col_f
  d_lx.alloc(sg.total());
  arslam::launch_pack(sg, d_lx.p, false, stream);
  allreduce(d_lx.p, sg.total(), ARSLAM_OP_SUM);
  arslam::launch_pack(sg, d_lx.p, true, stream);
  lin_norms();
}

// Several ranks: the scalars of fl (indices into d_red) and, if a
// linearization's norms are pending, its capture-slot norms, all-gathered in
// one SUM all-reduce and combined in rank order (k_ag_put / k_ag_reduce: the
// same bits on every rank); the norms then go to h_lin like the rest of it.
void arslam_lm::exchange_scalars(arslam::AgFields fl, arslam::HostOut *ho) {
  const bool with_norms = norms_pending;
  if (with_norms) {
    // the norms over the slots each rank holds (captures; its f-side slots)
    const int nb0 = (int)(d_norms_p - d_red.p);
    for (int q = 0; q < 6; ++q) fl.add(nb0 + q, q % 3 == 0);   // max |g|, sum g^2, sum x^2 (captures, then f-side)
    fl.add(kLinSave, false);       // the linearization's cost
    fl.add(kLinSave + 1, false);   // ... and fixed cost
  }
  if (fl.n == 0 && !ho) return;   // (with ho the combining launch still stores the host words)
  d_ag.alloc((size_t)nranks * arslam::kAgFields);
  arslam::launch_ag_put(d_red.p, fl, d_ag.p, nranks, rank, stream);
  allreduce(d_ag.p, (size_t)nranks * arslam::kAgFields, ARSLAM_OP_SUM);
  if (with_norms && ho) {   // (the combining launch stores them with the step's words)
    h_lin.alloc(32);
    ho->add(d_norms_p, h_lin.p + 16, 6);
    ho->add(d_red.p + kLinSave, h_lin.p, 2);
  }
  arslam::launch_ag_reduce(d_ag.p, fl, d_red.p, nranks, stream, ho);
  if (with_norms) {
    if (!ho) {
      HIP_CHECK(hipMemcpyAsync(h_lin.p + 16, d_norms_p, 6 * sizeof(double), hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipMemcpyAsync(h_lin.p, d_red.p + kLinSave, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    norms_pending = false;
  }
}

// (after a stream sync that covers linearize_launch)
void arslam_lm::linearize_collect(double *x_cost, double *fixed_cost, double *gmax, double *gnorm,
                                  double *xnorm) {
  const double *red = h_lin.p, *norms = h_lin.p + 16;
  *x_cost = red[arslam::P_COST];
  *fixed_cost = red[arslam::P_FIXED];
  *gmax = std::max(norms[0], norms[3]);
  *gnorm = std::sqrt(norms[1] + norms[4]);
  *xnorm = std::sqrt(norms[2] + norms[5]);
  timers[PH_LIN].collect();
}

// Evaluate residuals/Jacobian at x: cost, gradient (unscaled), column norms
// and the norms the minimizer reads.  Ceres EvaluateGradientAndJacobian.
void arslam_lm::linearize(double *x_cost, double *fixed_cost, double *gmax, double *gnorm,
                          double *xnorm) {
  linearize_launch();
  complete_pending_lin();
  exchange_norms();
  lin_sync();
  linearize_collect(x_cost, fixed_cost, gmax, gnorm, xnorm);
}

void arslam_lm::write_back(const double *d_src) {
  h_x.alloc(n + 1);   // page-locked; [n]: the download's sequence word (one rank)
  const bool dma = env.write_back_dma;   // debug A/B: the copy engine
  if (!multi() && !dma) {
    // a kernel stores x into h_x and then the sequence word the host polls
    // (the copy engine's download and an event behind it took ~70 us per
    // Solve on the incremental flow)
    const double seq = next_seq(h_x.p + n);
    arslam::launch_copy_out(d_src, n, h_x.p, d_seq_done.p, h_x.p + n, seq, stream);
    flag_sync(h_x.p + n, seq);
  } else {
    HIP_CHECK(hipMemcpyAsync(h_x.p, d_src, n * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  if (multi()) {
    // the camera and each tag from the rank holding it (the others hold stale
    // values of other ranks' subtree tags, and of the camera when its rows are
    // not in the replicated top -- a split with one active rank and no top):
    // one all-reduce of the held values, zeros elsewhere
    const long t0 = 3 + 6L * nc;
    d_lx.alloc(3 + n - t0);
    arslam::launch_own_copy(P, 0, 3, d_src, d_lx.p, stream);
    arslam::launch_own_copy(P, t0, n - t0, d_src + t0, d_lx.p + 3, stream);
    allreduce(d_lx.p, 3 + n - t0, ARSLAM_OP_SUM);
    HIP_CHECK(hipMemcpyAsync(h_x.p, d_lx.p, 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(h_x.p + t0, d_lx.p + 3, (n - t0) * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  if (multi() || dma) spin_sync();
  const double *h = h_x.p;
  std::memcpy(soa.camera, h, 3 * sizeof(double));
  if (elim_used == ARSLAM_ELIM_MIXED) {   // groups (not the direct ones: copies) and f-blocks to their blocks
    for (int g = 0; g < nc; ++g)
      if (mx.kind[g] != arslam::kMixDirect)
        std::memcpy((mx.kind[g] == arslam::kMixTag ? soa.tag : soa.cap) + 6L * mx.group_src[g], h + 3 + 6L * g,
                    6 * sizeof(double));
    for (int f = 0; f < nt; ++f)
      std::memcpy((mx.f_is_cap[f] ? soa.cap : soa.tag) + 6L * mx.f_src[f], h + 3 + 6L * nc + 6L * f,
                  6 * sizeof(double));
  } else if (multi()) {   // this rank's captures into the whole problem's array
    for (int c = 0; c < nc; ++c) std::memcpy(soa.cap + 6L * own_caps[c], h + 3 + 6L * c, 6 * sizeof(double));
  } else if (nc) {
    std::memcpy(soa.cap, h + 3, 6L * nc * sizeof(double));
  }
  if (nt && elim_used != ARSLAM_ELIM_MIXED) std::memcpy(soa.tag, h + 3 + 6L * nc, 6L * nt * sizeof(double));
  if (pk_stage) scatter_to_blocks();
}

// Pointer-keyed path: the staging arrays (which soa aliases, role-swapped or
// not) -> the caller's parameter blocks, as Ceres writes the user's blocks.
void arslam_lm::scatter_to_blocks() {
  const arslam_soa_problem &p = *pk_stage;
  std::memcpy(camera_ptr, p.camera, 3 * sizeof(double));
  for (size_t c = 0; c < cap_ptrs.size(); ++c) std::memcpy(cap_ptrs[c], p.cap + 6 * c, 6 * sizeof(double));
  for (size_t t = 0; t < tag_ptrs.size(); ++t) std::memcpy(tag_ptrs[t], p.tag + 6 * t, 6 * sizeof(double));
}

void arslam_lm::restore_patched_wait() {
  if (dbg_patched_wait < 0) return;
  const int w = dbg_patched_wait;
  dbg_patched_wait = -1;
  plan.h_dag_waits[w].y -= 1 << 28;
  HIP_CHECK(hipMemcpyAsync(plan.dag_waits + w, &plan.h_dag_waits[w], sizeof(int2), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
}

// Several ranks: every rank takes the same branch on the callbacks' answers
// (MAX over the ranks of continue 0 < terminate successfully 1 < abort 2).
int arslam_lm::agree_callback(int r) {
  if (!multi()) return r;
  const double v = r == ARSLAM_SOLVER_ABORT ? 2.0 : r == ARSLAM_SOLVER_TERMINATE_SUCCESSFULLY ? 1.0 : 0.0;
  d_cb.alloc(1);
  HIP_CHECK(hipMemcpyAsync(d_cb.p, &v, sizeof(double), hipMemcpyHostToDevice, stream));
  allreduce(d_cb.p, 1, ARSLAM_OP_MAX);
  double m = 0.0;
  HIP_CHECK(hipMemcpyAsync(&m, d_cb.p, sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  return m >= 2.0 ? ARSLAM_SOLVER_ABORT : m >= 1.0 ? ARSLAM_SOLVER_TERMINATE_SUCCESSFULLY : ARSLAM_SOLVER_CONTINUE;
}

namespace {

void print_header() {
  std::printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius  ls_iter  iter_time  total_time\n");
}

void print_row(const arslam_lm_iteration &it) {
  std::printf("% 4d % 8e   % 3.2e   % 3.2e  % 3.2e  % 3.2e % 3.2e     % 4d   % 3.2e   % 3.2e\n",
              it.iteration, it.cost, it.cost_change, it.gradient_max_norm, it.step_norm,
              it.relative_decrease, it.trust_region_radius, 0, it.iteration_time, it.cumulative_time);
  std::fflush(stdout);
}

}  // namespace

// ---- the stages of a solve ----
void arslam_lm::begin_solve(arslam_lm_summary *s) {
  std::memset(s, 0, sizeof(*s));
  for (auto &t : timers) {
    t.acc_ms = 0.0;
    t.on = opt.phase_timing != 0;
  }
  dom_ms = dom_flops = 0.0;
  dom_launches = 0;
  norms_pending = lin_xpending = false;
  s->n_obs = nb;
  s->n_reduced = has_f ? (int)nR : 0;
  s->setup_time_s = setup_s;
  for (int i = 0; i < 5; ++i) s->setup_phase_s[i] = setup_phase[i];
  s->setup_kind = setup_kind;
  x = d_xa.p;
  xc = d_xb.p;
  xbest = x;   // (iteration 0's finalize makes it so)
  HIP_CHECK(hipMemcpyAsync(x, u_x0, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  if (opt.minimizer_progress_to_stdout && rank == 0) print_header();
  // a callback on any rank: every rank joins the per-iteration agreement (the
  // same MAX all-reduce, of 1 for a callback and 0 for none)
  any_iter_cb = agree_callback(iter_cb ? ARSLAM_SOLVER_TERMINATE_SUCCESSFULLY : ARSLAM_SOLVER_CONTINUE) !=
                ARSLAM_SOLVER_CONTINUE;
  comm_bytes = 0.0;   // (the per-step exchange count starts here)
  comm_calls = 0;
}

// The executor reset / LM diagonal of a step.  The LM diagonal is current:
// k_scale formed it for the first step and every accepted step's
// linearization re-forms it (k_slot_norms); a rejected or invalid step keeps it.
bool arslam_lm::prepare_step(bool reuse_diag, arslam::ExecReset *er) {
  const bool exec_dag = has_f && opt.factor_executor == 1;
  if (exec_dag && nc > 0) {
    // flag + executor counters + the backward solve's y sentinels: in k_schur's launch
    *er = arslam::exec_reset_args(plan, d_flag.p, d_yF.p, nR);
    return true;
  }
  if (exec_dag) {
    const arslam::LmDiagArgs ld{0, d_scale.p, d_colnorm.p, opt.min_lm_diagonal, opt.max_lm_diagonal, d_diag.p, d_yF.p, nR};
    arslam::launch_exec_reset(plan, d_flag.p, stream, &ld);
  } else {
    if (!reuse_diag)
      arslam::launch_lm_diag(P, d_scale.p, d_colnorm.p, opt.min_lm_diagonal, opt.max_lm_diagonal, d_diag.p, stream);
    HIP_CHECK(hipMemsetAsync(d_flag.p, 0, sizeof(int), stream));
  }
  return false;
}

namespace {
bool g_dag_traced = false;   // ARSLAM_DAG_TRACE: one trace per process
int g_dag_trace_seen = 0;    // ... of the launch after ARSLAM_DAG_TRACE_SKIP others
}  // namespace

// ARSLAM_DAG_TRACE: one k_factor_dag launch stamping its tasks' times, and the
// file tools/dag_*.py and potrf_*.py read
void arslam_lm::dump_dag_trace(long first_store) {
  DevBuf<unsigned long long> tr;
  tr.alloc(arslam::kDagTraceWords * plan.n_dag_tasks);
  HIP_CHECK(hipMemsetAsync(tr.p, 0, tr.n * 8, stream));
  arslam::launch_dense_llt_dag(plan, Sp, d_flag.p, stream, dag_workgroups, nullptr, tr.p, false, -1, first_store);
  std::vector<unsigned long long> h(arslam::kDagTraceWords * plan.n_dag_tasks);
  HIP_CHECK(hipMemcpyAsync(h.data(), tr.p, h.size() * 8, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  if (FILE *f = std::fopen(env.dag_trace, "wb")) {
    const long n = plan.n_dag_tasks;
    std::fwrite(&n, 8, 1, f);
    std::fwrite(plan.h_dag_tasks.data(), sizeof(int4), n, f);
    // (a ticket's first kDagTraceFileWords words here; the rest in a block of their own at the end)
    for (long t = 0; t < n; ++t) std::fwrite(h.data() + t * arslam::kDagTraceWords, 8, arslam::kDagTraceFileWords, f);
    const long nw = (long)plan.h_dag_waits.size();   // the dependency lists, for dag_critical.py
    std::fwrite(&nw, 8, 1, f);
    std::fwrite(plan.h_dag_wait_off.data(), sizeof(int), n + 1, f);
    std::fwrite(plan.h_dag_waits.data(), sizeof(int2), nw, f);
    std::fwrite(plan.h_dag_sub.data(), sizeof(int2), n, f);   // fused TRSM tiles
    for (long t = 0; t < n; ++t)   // the stamps between a POTRF's two publishes, for potrf_cont.py
      std::fwrite(h.data() + t * arslam::kDagTraceWords + arslam::kDagTraceFileWords, 8, arslam::kDagTraceSubWords, f);
    std::fclose(f);
  }
  g_dag_traced = true;
}

void arslam_lm::factor_reduced(long first_store, bool record, double radius, bool force_indefinite) {
  if (opt.factor_executor != 1) {
    arslam::launch_dense_llt(plan, Sp, d_flag.p, stream, record ? &upd_timing : nullptr);
    return;
  }
  const bool rec = record && upd_timing.used < upd_timing.cap;
  if (rec) HIP_CHECK(hipEventRecord(upd_timing.ev[2 * upd_timing.used], stream));
  if (env.dag_trace && !g_dag_traced && g_dag_trace_seen++ >= env.dag_trace_skip) {
    dump_dag_trace(first_store);
  } else if (multi()) {
    // phase 0: this rank's subtree columns, and their updates of the top
    // tiles (its share of the top's Schur complement); then the top tiles
    // are summed over the ranks -- the step's one bulk exchange -- and
    // every rank factors the top columns (phase 1) on identical inputs
    timers[PH_FAC0].start(stream);
    arslam::launch_dense_llt_dag(plan, Sp, d_flag.p, stream, dag_workgroups, nullptr, nullptr, false, 0);
    timers[PH_FAC0].stop(stream);
    // (+ a pending linearization's top-tag sums and camera partials, in
    // front of the top tiles: the step's collectives stay two)
    const long tail = lin_xpending ? top_tail_len() : 0;
    if (tail) arslam::launch_top_tail(u_top_slots, n_top_slots, d_g.p, d_colnorm.p, d_red.p, Sp - tail, false, stream);
    allreduce(Sp - tail, (size_t)tail + (size_t)plan.n_top_tiles * 4096, ARSLAM_OP_SUM);
    if (tail) {
      arslam::launch_top_tail(u_top_slots, n_top_slots, d_g.p, d_colnorm.p, d_red.p, Sp - tail, true, stream);
      lin_norms();   // the LM diagonal of the top rows, then their D^2
    }
    arslam::launch_prep_reduced(P, d_diag.p, radius, Sp, stream, 1);
    if (force_indefinite)   // test hook (a top row)
      arslam::debug_set_reduced_diag(P, Sp, P.cam_row >= 0 ? P.cam_row : nR - 1, -1.0, stream);
    timers[PH_FAC1].start(stream);
    arslam::launch_dense_llt_dag(plan, Sp, d_flag.p, stream, dag_workgroups, nullptr, nullptr, false, 1);
    timers[PH_FAC1].stop(stream);
  } else {
    arslam::launch_dense_llt_dag(plan, Sp, d_flag.p, stream, dag_workgroups, nullptr, nullptr, false, -1, first_store);
  }
  if (rec) {
    HIP_CHECK(hipEventRecord(upd_timing.ev[2 * upd_timing.used + 1], stream));
    upd_timing.used++;
    upd_timing.flops += plan.total_factor_flops;
  }
}

// y of the reduced system, then the candidate xc = x + step and its cost per capture
void arslam_lm::back_substitute(double radius) {
  if (has_f) {
    timers[PH_SOLVE].start(stream);
    if (opt.factor_executor == 1)
      arslam::launch_dense_back_solve_dag(plan, Sp, nR, d_yF.p, d_flag.p, stream, dag_workgroups, false);
    else
      arslam::launch_dense_back_solve(plan, Sp, nR, d_z.p, d_yF.p, d_flag.p, stream);
    if (multi()) {
      // y of the top columns (identical on every rank) and of this rank's
      // own subtrees; no exchange: a rank's captures see only those tags
      // (a capture's tags lie on one root path of the elimination tree), so
      // each rank updates the tags it holds and keeps the others' stale,
      // and the sums over f-side slots count each slot on its holder
      // (DevProblem::f_own); the final tags are gathered in write_back
      arslam::launch_mask_y(P, d_yF.p, rank, stream, true);
    }
    timers[PH_SOLVE].stop(stream);
  }
  timers[PH_BACK].start(stream);
  // (k_update_f writes every f-side slot of xc, k_backsub every capture
  // slot, then evaluates the candidate's cost per capture: k_cost fused)
  arslam::launch_update_f(P, x, d_scale.p, d_yF.p, xc, d_fparts.p, stream);
  arslam::launch_backsub(P, x, d_scale.p, d_diag.p, radius, d_yF.p, xc, d_parts.p, stream, has_f, true, cl());
  timers[PH_BACK].stop(stream);
}

// the step's scalars into h_step, its sequence word last: returns the number to wait for
double arslam_lm::reduce_step_scalars() {
  timers[PH_COST].start(stream);
  h_step.alloc(16);
  // (one rank: the scalars are also stored straight into the page-locked h_step)
  double step_seq = !multi() ? next_seq(h_step.p + arslam::kHostSeq) : 0.0;
  arslam::launch_reduce_parts(d_parts.p, nc, d_fparts.p, n_fparts, d_red.p, stream, d_flag.p,
                              !multi() ? h_step.p : nullptr, d_seq_done.p, step_seq);
  if (multi()) {
    // candidate cost, fixed, model change, capture step^2 by sum; the
    // non-finite flags, the f-side non-finite step, indefinite and executor
    // fault by max (every rank takes the same branch); with a pending
    // linearization's norms: one collective
    arslam::AgFields fl;
    for (int f : {(int)arslam::P_COST, (int)arslam::P_FIXED, (int)arslam::P_MODEL, (int)arslam::P_STEP2,
                  (int)arslam::NPART})   // (NPART: the f-side step^2, of the slots this rank holds)
      fl.add(f, false);
    for (int f : {(int)arslam::P_YBAD, (int)arslam::P_CBAD, arslam::NPART + 1, arslam::NPART + 2, arslam::NPART + 3})
      fl.add(f, true);
    // the step's words (and a pending linearization's norms) stored to the
    // host by the combining launch, then its sequence number
    arslam::HostOut ho;
    ho.add(d_red.p, h_step.p, arslam::NPART + 5);
    step_seq = next_seq(h_step.p + arslam::kHostSeq);
    ho.seq_word = h_step.p + arslam::kHostSeq;
    ho.seq = step_seq;
    exchange_scalars(fl, &ho);
  }
  timers[PH_COST].stop(stream);
  return step_seq;
}

// ---- ComputeTrustRegionStep: LM diagonal, DENSE_SCHUR solve ----
double arslam_lm::enqueue_step(double radius, bool reuse_diag, int solve_index) {
  arslam::ExecReset er{};
  const bool reset_in_schur = prepare_step(reuse_diag, &er);
  // several ranks: a pending linearization's sums ride with the top tiles
  // (factor_reduced), unless this step has no such exchange
  if (lin_xpending && !(has_f && opt.factor_executor == 1 && !env.dag_trace)) complete_pending_lin();
  if (has_f) {
    timers[PH_SCHUR].start(stream);
    // one rank: the gather writes the final S (D_f^2 and the padding rows
    // included).  Several: this rank's captures' share; the D_f^2 of the
    // rank's own subtree rows now, of the top rows after their exchange
    // (factor_reduced).  k_schur's extra blocks clear S's tiles first.
    // (one rank on the persistent executor: the fill tiles the gather does
    // not write are left as they are -- their first update stores)
    const bool fill_first_store = !multi() && opt.factor_executor == 1;
    arslam::launch_schur(P, x, d_scale.p, d_diag.p, radius, Sp, stream, !multi(),
                         fill_first_store ? n_clear : plan.n_tiles, reset_in_schur ? &er : nullptr);
    // (l1, l2 estimated: their border of the Schur complement, after the gather)
    if (est_loaded) arslam::launch_schur_cam(P, CL, d_scale.p, d_diag.p, radius, Sp, stream);
    const bool force_indefinite = dbg_indefinite_mask >> std::min(solve_index, 63) & 1ull;
    if (multi()) arslam::launch_prep_reduced(P, d_diag.p, radius, Sp, stream, 0);
    else if (force_indefinite)   // test hook
      arslam::debug_set_reduced_diag(P, Sp, P.cam_row >= 0 ? P.cam_row : nR - 1, -1.0, stream);
    timers[PH_SCHUR].stop(stream);
    timers[PH_CHOL].start(stream);
    timing_begin();
    factor_reduced(fill_first_store ? n_clear : LONG_MAX, opt.kernel_timing != 0, radius, force_indefinite);
    timers[PH_CHOL].stop(stream);
  }
  back_substitute(radius);
  return reduce_step_scalars();
}

void arslam_lm::fill_summary(arslam_lm_summary *s) {
  const long nb_all = nb_global;
  s->n_obs = (int)nb_all;
  s->final_rms_px = nb_all ? std::sqrt(2.0 * s->final_cost / (4.0 * nb_all)) : 0.0;
  s->t_linearize_ms = timers[PH_LIN].acc_ms;
  s->t_schur_ms = timers[PH_SCHUR].acc_ms;
  s->t_cholesky_ms = timers[PH_CHOL].acc_ms;
  s->t_solve_ms = timers[PH_SOLVE].acc_ms;
  s->t_backsub_ms = timers[PH_BACK].acc_ms;
  s->t_cost_ms = timers[PH_COST].acc_ms;
  s->t_factor_own_ms = timers[PH_FAC0].acc_ms;
  s->t_factor_top_ms = timers[PH_FAC1].acc_ms;
  s->t_dominant_ms = dom_ms;
  s->dominant_flops = dom_flops;
  s->n_dominant_launches = dom_launches;
  s->n_factor_tiles = plan.n_tiles;
  s->n_levels = plan.nlev;
  s->n_update_tiles = plan.total_upd_tiles;
  s->factor_update_flops = plan.total_upd_flops;
  s->factor_scalar_flops = scalar_flops;
  s->comm_bytes = comm_bytes;
  s->comm_calls = comm_calls;
  s->elimination_used = elim_used;
  s->ceres_e_captures = ceres_e_cap;
  s->ceres_e_tags = ceres_e_tag;
  s->n_ranks = nranks;
  s->n_owned_captures = multi() ? nc : nc_user;   // (one rank: every capture, whichever side is eliminated)
  s->n_top_tiles = multi() ? plan.n_top_tiles : 0;
  s->split_top_work = split_top_work;
  s->split_max_rank_work = split_max_rank_work;
  s->split_total_work = split_total_work;
  s->n_active_ranks = multi() ? split_active : 1;
  s->order_reused = order.last_reused ? 1 : 0;
}

namespace {

// Ceres' trust-region scalars: LevenbergMarquardtStrategy's radius and
// decrease factor, whether the LM diagonal in d_diag is still the current
// point's, and the minimizer's count of consecutive invalid steps.
struct TrustRegion {
  double radius;
  double decrease_factor = 2.0;
  bool reuse_diag = false;
  int n_invalid = 0;
  void shrink(int invalid) {   // StepRejected; StepIsInvalid
    n_invalid = invalid;
    radius = radius / decrease_factor;
    decrease_factor *= 2.0;
    reuse_diag = true;
  }
  void invalid() { shrink(n_invalid + 1); }
  void rejected() { shrink(0); }
  void accepted(double rho, double max_radius) {   // StepAccepted
    n_invalid = 0;
    const double q = 2.0 * rho - 1.0;
    radius = radius / std::max(1.0 / 3.0, 1.0 - q * q * q);
    radius = std::min(max_radius, radius);
    decrease_factor = 2.0;
    reuse_diag = false;
  }
};

// the two guards of a solve, each for the whole of it, exceptional exit included:
// the patched dependency of arslam_lm_debug_break_dependency lasts one solve
struct RestoreWait {
  arslam_lm *h;
  ~RestoreWait() {
    try { h->restore_patched_wait(); } catch (...) {}
  }
};
// ... and diag_in_lin is off again when the solve ends, however it ends
struct DiagInLin {
  arslam_lm *h;
  ~DiagInLin() { h->diag_in_lin = false; }
};

}  // namespace

void arslam_lm::solve(arslam_lm_summary *s) {
  fail_if(!loaded, ARSLAM_E_STATE, "no problem loaded");
  cov_invalidate();
  const arslam_lm_options &o = opt;
  const double t_start = now_s();
  RestoreWait restore_wait{this};
  begin_solve(s);
  const bool root = rank == 0;
  const auto stop = [s](int termination, int rule) {   // (true: the minimizer stops)
    s->termination = termination;
    s->rule = rule;
    return true;
  };

  // ---- iteration 0 ----
  double x_cost, fixed_cost, gmax, gnorm, x_norm;
  linearize(&x_cost, &fixed_cost, &gmax, &gnorm, &x_norm);
  s->fixed_cost = fixed_cost;
  s->initial_cost = x_cost + fixed_cost;
  s->final_cost = s->initial_cost;
  if (!std::isfinite(x_cost)) {
    stop(ARSLAM_FAILURE, ARSLAM_RULE_EVAL_FAILED);
    s->total_time_s = now_s() - t_start;
    solve_state = 2;
    return;
  }
  // the scale, and from it the first step's LM diagonal (k_lm_diag's work)
  const arslam::LmDiagArgs ld{n, d_scale.p, d_colnorm.p, o.min_lm_diagonal, o.max_lm_diagonal, d_diag.p};
  arslam::launch_scale(P, d_colnorm.p, o.jacobi_scaling, d_scale.p, stream, &ld);
  diag_in_lin = true;
  DiagInLin diag_in_lin_guard{this};

  TrustRegion tr{o.initial_trust_region_radius};
  double minimum_cost = x_cost;
  arslam_lm_iteration it{};
  it.iteration = 0;
  it.cost = x_cost + fixed_cost;
  it.gradient_max_norm = gmax;
  it.gradient_norm = gnorm;
  it.step_is_valid = 1;
  it.step_is_successful = 1;
  double t_iter = t_start;

  // A successful step's re-linearization is only enqueued (lin_pending): the
  // next step's kernels follow it in the stream, and its results are read at
  // that step's one host sync, where the finalization below runs first.  If
  // it then stops the minimizer, the speculative step is dropped uncounted.
  bool lin_pending = false;
  double prev_gmax = 0.0, prev_gnorm = 0.0;
  auto finalize = [&]() -> bool {   // true: the minimizer stops
    if (lin_pending) {
      double fc;
      linearize_collect(&x_cost, &fc, &gmax, &gnorm, &x_norm);
      it.cost = x_cost + fixed_cost;
      it.gradient_max_norm = gmax;
      it.gradient_norm = gnorm;
      lin_pending = false;
    }
    // ---- FinalizeIterationAndCheckIfMinimizerCanContinue ----
    if (it.step_is_successful) {
      if (it.iteration > 0) s->num_successful_steps++;
      if (x_cost < minimum_cost || it.iteration == 0) {
        minimum_cost = x_cost;
        xbest = x;   // (by pointer: no copy; the step in flight writes xc)
        if (o.update_state_every_iteration) write_back(xbest);
      }
    } else {
      s->num_unsuccessful_steps++;
    }
    it.trust_region_radius = tr.radius;
    const double tn = now_s();
    it.iteration_time = tn - t_iter;
    it.cumulative_time = tn - t_start;
    t_iter = tn;
    if (s->n_iters <= ARSLAM_LM_MAX_ITERS) s->iters[s->n_iters++] = it;
    if (o.minimizer_progress_to_stdout && root) print_row(it);
    if (iter_cb || any_iter_cb) {   // Ceres RunCallbacks: after the record, before the stop rules
      const int r = agree_callback(iter_cb ? iter_cb(iter_cb_ctx, &it) : ARSLAM_SOLVER_CONTINUE);
      if (r == ARSLAM_SOLVER_ABORT) return stop(ARSLAM_USER_FAILURE, ARSLAM_RULE_USER_CALLBACK);
      if (r == ARSLAM_SOLVER_TERMINATE_SUCCESSFULLY) return stop(ARSLAM_USER_SUCCESS, ARSLAM_RULE_USER_CALLBACK);
    }
    if (it.iteration >= o.max_num_iterations) return stop(ARSLAM_NO_CONVERGENCE, ARSLAM_RULE_MAX_ITERS);
    if (it.step_is_successful && it.gradient_max_norm <= o.gradient_tolerance)
      return stop(ARSLAM_CONVERGENCE, ARSLAM_RULE_GRADIENT);
    if (tr.radius <= o.min_trust_region_radius) return stop(ARSLAM_CONVERGENCE, ARSLAM_RULE_MIN_RADIUS);
    prev_gmax = it.gradient_max_norm;
    prev_gnorm = it.gradient_norm;
    const int next_iter = it.iteration + 1;
    it = arslam_lm_iteration{};
    it.iteration = next_iter;
    return false;
  };

  for (;;) {
    // the stop rules that do not read the pending linearization: decided now
    // (after reading it), so no step is computed past them
    const bool stop_rule = it.iteration >= o.max_num_iterations || tr.radius <= o.min_trust_region_radius;
    if (lin_pending && stop_rule) {
      complete_pending_lin();
      exchange_norms();
      lin_sync();
    }
    const bool deferred = lin_pending && !stop_rule;
    if (!deferred && finalize()) break;

    // ---- ComputeTrustRegionStep: one host round trip ----
    const double step_seq = enqueue_step(tr.radius, tr.reuse_diag, s->num_linear_solves++);
    flag_sync(h_step.p + arslam::kHostSeq, step_seq);
    const double *red = h_step.p;
    // A stuck dependency wait of a persistent executor is a device fault, not
    // an indefinite system: fail loudly instead of shrinking the radius.
    if (red[arslam::NPART + 3] != 0.0)
      throw Error(ARSLAM_E_DEVICE, executor_fault_message((int)red[arslam::NPART + 4], rank, it.iteration, plan, stream));
    for (int ph = PH_SCHUR; ph < PH_N; ++ph) timers[ph].collect();
    timing_collect();
    if (deferred && finalize()) {
      s->num_linear_solves--;   // the speculative step is not part of the trace
      break;
    }

    const bool lin_fail = red[arslam::NPART + 2] != 0.0;   // LLT failure: Ceres' invalid step
    const bool ybad = red[arslam::P_YBAD] != 0.0 || red[arslam::NPART + 1] != 0.0;
    const double model_cost_change = red[arslam::P_MODEL];
    const bool valid = !lin_fail && !ybad && model_cost_change > 0.0;
    if (!valid) {
      // Ceres 2.0 HandleInvalidStep: ++num_consecutive_invalid_steps_ >= max -> FAILURE
      // (the 5th consecutive invalid step at the default 5, not recorded)
      tr.invalid();
      if (tr.n_invalid >= o.max_num_consecutive_invalid_steps) { stop(ARSLAM_FAILURE, ARSLAM_RULE_INVALID_STEPS); break; }
      it.cost = x_cost + fixed_cost;
      it.gradient_max_norm = prev_gmax;
      it.gradient_norm = prev_gnorm;
      it.step_is_valid = 0;
      it.step_is_successful = 0;
      continue;
    }
    it.step_is_valid = 1;
    double candidate_cost = red[arslam::P_COST];
    if (!std::isfinite(candidate_cost) || red[arslam::P_CBAD] != 0.0) candidate_cost = DBL_MAX;
    it.step_norm = std::sqrt(red[arslam::P_STEP2] + red[arslam::NPART]);
    // ---- ParameterToleranceReached ----
    if (it.step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) {
      stop(ARSLAM_CONVERGENCE, ARSLAM_RULE_PARAMETER); break;
    }
    // ---- FunctionToleranceReached ----
    it.cost_change = x_cost - candidate_cost;
    if (std::fabs(it.cost_change) <= o.function_tolerance * x_cost) {
      stop(ARSLAM_CONVERGENCE, ARSLAM_RULE_FUNCTION); break;
    }
    // ---- IsStepSuccessful ----
    it.relative_decrease = candidate_cost >= DBL_MAX ? -DBL_MAX
                                                     : (x_cost - candidate_cost) / model_cost_change;
    if (it.relative_decrease > o.min_relative_decrease) {
      // the candidate becomes x; the next candidate goes to a buffer that is
      // neither x nor the best point (the old x, unless it is the best: its
      // successor's cost is read only at the next sync, after the next step
      // is enqueued)
      double *old = x;
      x = xc;
      xc = old != xbest ? old : (d_xa.p != x && d_xa.p != xbest) ? d_xa.p : (d_xb.p != x && d_xb.p != xbest) ? d_xb.p : d_xbest.p;
      linearize_launch();   // read at the next step's sync (finalize)
      lin_pending = true;
      it.step_is_successful = 1;
      tr.accepted(it.relative_decrease, o.max_trust_region_radius);
    } else {
      it.step_is_successful = 0;
      tr.rejected();
      it.cost = candidate_cost + fixed_cost;
      it.gradient_max_norm = prev_gmax;
      it.gradient_norm = prev_gnorm;
    }
  }
  s->final_cost = minimum_cost + fixed_cost;
  s->minimizer_time_s = now_s() - t_start;
  write_back(xbest);
  s->total_time_s = now_s() - t_start;
  if (env.setup_profile) std::fprintf(stderr, "arslam write_back %.3f ms\n", 1e3 * (s->total_time_s - s->minimizer_time_s));
  fill_summary(s);
  solve_state = 1;
}
