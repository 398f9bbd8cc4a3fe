// lm_capi.hip -- the C-ABI of include/arslam_lm.h over the LM handle
// (lm_handle.h): argument checks, the pointer-keyed problem's staging, and
// the translation of exceptions into error codes (api_guarded).  The
// covariance entry points are lm_cov_capi.hip's.
#include "lm_handle.h"

arslam_lm::~arslam_lm() {
  for (auto &t : timers) t.destroy();
  for (auto e : upd_events) (void)hipEventDestroy(e);
  if (ev_sync) (void)hipEventDestroy(ev_sync);
  for (auto e : cov_ev)
    if (e) (void)hipEventDestroy(e);
  arslam::selinv_plan_free(cov_sp);
  for (auto e : pair_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto e : ev_evt)
    if (e) (void)hipEventDestroy(e);
  arslam::tile_solve_plan_free(cov_tp);
  arslam::llt_plan_free(plan);
  if (comm) (void)ncclCommDestroy(comm);
  if (stream) (void)hipStreamDestroy(stream);
}

// ===========================================================================
// C-ABI
// ===========================================================================

namespace {
thread_local std::string g_last_error;
}  // namespace
namespace arslam {
void set_last_error(const std::string &msg) { g_last_error = msg; }
}  // namespace arslam

extern "C" {

int arslam_lm_options_init(arslam_lm_options *o) {
  if (!o) return ARSLAM_E_INVALID_ARG;
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 50;              // ar_slam_util.cpp:1004
  o->function_tolerance = 1e-6;            // Ceres 2.0 defaults below
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->elimination = ARSLAM_ELIM_AUTO;       // DENSE_SCHUR, ar_slam_util.cpp:1011
  o->minimizer_progress_to_stdout = 0;
  o->update_state_every_iteration = 0;
  o->device = -1;
  o->cholesky_skip_zero_tiles = 1;
  o->reduced_ordering = 2;
  o->kernel_timing = 0;
  o->factor_executor = 1;
  o->phase_timing = 0;
  return ARSLAM_OK;
}

int arslam_lm_create(arslam_lm **out, const arslam_lm_options *opt) {
  if (!out) return ARSLAM_E_INVALID_ARG;
  *out = nullptr;
  return arslam::api_guarded([&] {
    auto *h = new arslam_lm();
    if (opt) h->opt = *opt; else arslam_lm_options_init(&h->opt);
    if (h->opt.elimination < ARSLAM_ELIM_AUTO || h->opt.elimination > ARSLAM_ELIM_MIXED) {
      delete h;
      throw Error(ARSLAM_E_INVALID_ARG, "elimination must be ARSLAM_ELIM_AUTO, _CAPTURES, _TAGS or _MIXED");
    }
    *out = h;
  });
}

void arslam_lm_destroy(arslam_lm *h) { delete h; }

int arslam_lm_set_options(arslam_lm *h, const arslam_lm_options *opt) {
  if (!h || !opt) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(opt->elimination < ARSLAM_ELIM_AUTO || opt->elimination > ARSLAM_ELIM_MIXED, ARSLAM_E_INVALID_ARG,
            "elimination must be ARSLAM_ELIM_AUTO, _CAPTURES, _TAGS or _MIXED");
    fail_if(opt->factor_executor != 0 && opt->factor_executor != 1, ARSLAM_E_INVALID_ARG,
            "factor_executor must be 0 or 1");
    fail_if(opt->max_num_iterations < 0 || opt->max_num_iterations > ARSLAM_LM_MAX_ITERS,
            ARSLAM_E_INVALID_ARG, "max_num_iterations out of range");
    // the stream and every device buffer live on the device of the first load
    fail_if(h->stream && opt->device >= 0 && opt->device != h->device,
            ARSLAM_E_INVALID_ARG, "a handle's device is fixed once it has loaded a problem: create a new handle");
    if (opt->device != h->opt.device || opt->reduced_ordering != h->opt.reduced_ordering ||
        opt->cholesky_skip_zero_tiles != h->opt.cholesky_skip_zero_tiles || opt->elimination != h->opt.elimination)
      h->loaded = false, h->pk_dirty = true, h->eval_drop();
    h->opt = *opt;
  });
}

int arslam_lm_get_options(const arslam_lm *h, arslam_lm_options *opt) {
  if (!h || !opt) return ARSLAM_E_INVALID_ARG;
  *opt = h->opt;
  return ARSLAM_OK;
}

int arslam_lm_set_loss(arslam_lm *h, int kind, double a) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!arslam::loss_valid(kind, a), ARSLAM_E_INVALID_ARG,
            "loss: kind must be ARSLAM_LOSS_NONE, _HUBER, _SOFT_L_ONE or _CAUCHY, its scale finite and > 0");
    h->def_loss_kind = kind;
    h->def_loss_a = kind == ARSLAM_LOSS_NONE ? 0.0 : a;
    // (the pointer-keyed blocks keep the losses they were added with; the
    // resident problem is dropped all the same: one rule for both paths)
    h->loaded = false;
    h->pk_dirty = true;
    h->eval_drop();
  });
}

int arslam_lm_get_loss(const arslam_lm *h, int *kind, double *a) {
  if (!h || !kind || !a) return ARSLAM_E_INVALID_ARG;
  *kind = h->def_loss_kind;
  *a = h->def_loss_a;
  return ARSLAM_OK;
}

int arslam_lm_set_tag_size(arslam_lm *h, double size) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!arslam::tag_size_valid(size), ARSLAM_E_INVALID_ARG, "tag size: finite and > 0 (metres)");
    h->def_tag_size = size;
    // (as arslam_lm_set_loss: the blocks keep the sides they were added with,
    // the resident problem is dropped)
    h->loaded = false;
    h->pk_dirty = true;
    h->eval_drop();
  });
}

int arslam_lm_get_tag_size(const arslam_lm *h, double *size) {
  if (!h || !size) return ARSLAM_E_INVALID_ARG;
  *size = h->def_tag_size;
  return ARSLAM_OK;
}

int arslam_lm_set_camera_model(arslam_lm *h, int model) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!ARSLAM_CAMERA_MODEL_VALID(model), ARSLAM_E_INVALID_ARG,
            "camera model: ARSLAM_CAMERA_PINHOLE or ARSLAM_CAMERA_RADIAL");
    if (model == h->camera_model) return;
    fail_if(model == ARSLAM_CAMERA_RADIAL && h->estimate_distortion && h->multi(), ARSLAM_E_UNSUPPORTED,
            "estimate_distortion is single-rank only: ARSLAM_CAMERA_RADIAL with it on a handle of several ranks");
    h->camera_model = model;
    // (as arslam_lm_set_tag_size: the resident problem was linearized under the
    // other model; so was its last solve, which a kept covariance describes)
    h->loaded = false;
    h->pk_dirty = true;
    h->eval_drop();
    h->cov_invalidate();
  });
}

int arslam_lm_camera_model(const arslam_lm *h, int *model) {
  if (!h || !model) return ARSLAM_E_INVALID_ARG;
  *model = h->camera_model;
  return ARSLAM_OK;
}

int arslam_lm_set_estimate_distortion(arslam_lm *h, int on) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(on != 0 && on != 1, ARSLAM_E_INVALID_ARG, "estimate_distortion: 0 or 1");
    if (on == h->estimate_distortion) return;
    fail_if(on && h->camera_model == ARSLAM_CAMERA_RADIAL && h->multi(), ARSLAM_E_UNSUPPORTED,
            "estimate_distortion is single-rank only (the l1, l2 rows have no rank exchange)");
    h->estimate_distortion = on;
    // (as arslam_lm_set_camera_model: the resident problem and its last solve
    // had the other set of parameters)
    h->loaded = false;
    h->pk_dirty = true;
    h->eval_drop();
    h->cov_invalidate();
  });
}

int arslam_lm_estimate_distortion(const arslam_lm *h, int *on) {
  if (!h || !on) return ARSLAM_E_INVALID_ARG;
  *on = h->estimate_distortion;
  return ARSLAM_OK;
}

int arslam_lm_debug_camera_rows(arslam_lm *h, double radius, long n_cols, double *rows, int *row_slot) {
  if (!h || !rows || !(radius > 0.0)) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!h->loaded || h->multi() || !h->has_f || h->P.cam_row < 0, ARSLAM_E_STATE,
            "camera_rows: a one-rank problem loaded with a free camera");
    fail_if(n_cols != h->nR + 1, ARSLAM_E_INVALID_ARG, "camera_rows: n_cols must be the reduced row count + 1");
    h->ensure_stream();
    h->cov_invalidate();
    // as solve()'s iteration 0 and its first step up to the factorization
    h->x = h->d_xa.p;
    h->xc = h->d_xb.p;
    h->xbest = h->x;
    HIP_CHECK(hipMemcpyAsync(h->x, h->u_x0, h->n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    for (auto &t : h->timers) t.on = false;
    double c0, c1, c2, c3, c4;
    h->linearize(&c0, &c1, &c2, &c3, &c4);
    const arslam::LmDiagArgs ld{h->n, h->d_scale.p, h->d_colnorm.p, h->opt.min_lm_diagonal, h->opt.max_lm_diagonal,
                                h->d_diag.p};
    arslam::launch_scale(h->P, h->d_colnorm.p, h->opt.jacobi_scaling, h->d_scale.p, h->stream, &ld);
    arslam::launch_schur(h->P, h->x, h->d_scale.p, h->d_diag.p, radius, h->Sp, h->stream, true, h->plan.n_tiles);
    if (h->est_loaded) arslam::launch_schur_cam(h->P, h->CL, h->d_scale.p, h->d_diag.p, radius, h->Sp, h->stream);
    DevBuf<double> d_out;
    d_out.alloc(3 * n_cols);
    arslam::debug_cam_rows(h->P, h->Sp, d_out.p, h->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(rows, d_out.p, 3 * n_cols * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (row_slot)
      for (int b = 0; b < 3; ++b) row_slot[b] = h->lay.row_slot[h->P.cam_row + b];
  });
}

}  // extern "C"

namespace {
// the caller's slot (camera 3, captures 6 each, tags 6 each) of each slot of the
// loaded device problem, -1 for a direct group's copy of its capture; returns
// the caller's slot count
long caller_slots(const arslam_lm *h, const arslam_lm::BlockMap &bm, std::vector<long> &map) {
  map.assign(h->n, -1);
  for (int j = 0; j < 3; ++j) map[j] = j;
  for (long b = 0; b < (long)bm.n_cap + bm.n_tag; ++b) {   // the caller's blocks: captures, then tags
    const bool cap = b < bm.n_cap;
    const long dev = bm.device_block(cap, (int)(cap ? b : b - bm.n_cap), h->nc);
    for (int j = 0; j < 6 && dev >= 0; ++j) map[3 + 6 * dev + j] = 3 + 6 * b + j;
  }
  return 3 + 6L * (bm.n_cap + bm.n_tag);
}

// ... and of a sharded handle's: its captures are own_caps (the ranks eliminate
// captures), every tag is loaded on every rank
long caller_slots_sharded(const arslam_lm *h, std::vector<long> &map) {
  const long t0 = 3 + 6L * h->nc, t0_full = 3 + 6L * h->nc_full;
  map.assign(h->n, -1);
  for (int j = 0; j < 3; ++j) map[j] = j;
  for (long c = 0; c < h->nc; ++c)
    for (int j = 0; j < 6; ++j) map[3 + 6 * c + j] = 3 + 6L * h->own_caps[c] + j;
  for (long sl = t0; sl < h->n; ++sl) map[sl] = t0_full + (sl - t0);
  return t0_full + 6L * h->nt;
}

// The body of arslam_lm_debug_step_stages and _sharded: the launches of
// solve()'s iteration 0 and first step from the loaded point, the copy of S
// before the factorization, and the outputs by the caller's slots (map; rows:
// the layout's row_slot).  info's n, n_cap, n_tag, elimination_used and n_direct
// are the caller's.  lin_ride (a sharded handle): iteration 0's sums are final
// (the packed exchange) as in solve(); with it a linearization at the same point
// is enqueued again as after an accepted step, and its top-tag sums and camera
// partials ride in front of the top tiles, its cost and norms with the step's
// scalars (enqueue_step's path when a step follows).
void step_stages(arslam_lm *h, double radius, bool lin_ride, const std::vector<long> &map, const std::vector<int> &rows,
                 arslam_lm_step_info *info, double *g, double *colnorm, double *scale, double *diag, double *S,
                 int *row_slot, double *y, double *xc) {
  const bool sharded = h->multi();
  info->n_reduced = h->has_f ? h->nR : 0;
  info->n_padded = h->has_f ? h->P.N : 0;
  info->cam_row = h->has_f ? h->P.cam_row : -1;
  info->n_groups = h->nc;
  info->n_big_groups = h->P.n_big_caps;
  info->n_chunk_groups = h->P.n_chunk_caps;
  info->n_split_dest = h->has_f ? h->P.n_splits : 0;
  info->max_contrib = h->has_f ? h->sg.max_contrib : 0;
  info->n_tiles = h->has_f ? h->plan.n_tiles : 0;
  info->n_assembled_tiles = h->has_f ? h->plan.n_assembled : 0;
  // as solve()'s iteration 0 ...
  h->norms_pending = h->lin_xpending = false;
  h->x = h->d_xa.p;
  h->xc = h->d_xb.p;
  h->xbest = h->x;
  HIP_CHECK(hipMemcpyAsync(h->x, h->u_x0, h->n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  for (auto &t : h->timers) t.on = false;
  double gmax, gnorm, xnorm;
  h->linearize(&info->cost, &info->fixed_cost, &gmax, &gnorm, &xnorm);
  const arslam::LmDiagArgs ld{h->n, h->d_scale.p, h->d_colnorm.p, h->opt.min_lm_diagonal, h->opt.max_lm_diagonal,
                              h->d_diag.p};
  arslam::launch_scale(h->P, h->d_colnorm.p, h->opt.jacobi_scaling, h->d_scale.p, h->stream, &ld);
  struct DiagInLin {   // (as solve()'s guard)
    arslam_lm *h;
    ~DiagInLin() { h->diag_in_lin = false; }
  } diag_in_lin_guard{h};
  if (sharded && lin_ride) {
    h->diag_in_lin = true;
    h->linearize_launch();
  }
  // ... and enqueue_step's launches for its first step, every tile cleared,
  // with the copy of S between the assembly and the factorization
  arslam::ExecReset er{};
  const bool reset_in_schur = h->prepare_step(false, &er);
  if (h->lin_xpending && !(h->has_f && h->opt.factor_executor == 1 && !h->env.dag_trace)) h->complete_pending_lin();
  DevBuf<double> d_dense;
  const long N = info->n_padded;
  if (h->has_f) {
    arslam::launch_schur(h->P, h->x, h->d_scale.p, h->d_diag.p, radius, h->Sp, h->stream, !sharded, h->plan.n_tiles,
                         reset_in_schur ? &er : nullptr);
    if (h->est_loaded) arslam::launch_schur_cam(h->P, h->CL, h->d_scale.p, h->d_diag.p, radius, h->Sp, h->stream);
    if (sharded) arslam::launch_prep_reduced(h->P, h->d_diag.p, radius, h->Sp, h->stream, 0);
    if (S) {
      d_dense.alloc(N * N);
      arslam::debug_reduced_dense(h->P, h->Sp, d_dense.p, h->stream);
    }
    h->factor_reduced(LONG_MAX, false, radius);
  }
  h->back_substitute(radius);
  const double seq = h->reduce_step_scalars();
  HIP_CHECK(hipGetLastError());
  h->flag_sync(h->h_step.p + arslam::kHostSeq, seq);
  const double *red = h->h_step.p;
  if (red[arslam::NPART + 3] != 0.0)
    throw Error(ARSLAM_E_DEVICE, executor_fault_message((int)red[arslam::NPART + 4], h->rank, 0, h->plan, h->stream));
  info->model_cost_change = red[arslam::P_MODEL];
  info->candidate_cost = red[arslam::P_COST];
  info->candidate_fixed_cost = red[arslam::P_FIXED];
  info->e_step2 = red[arslam::P_STEP2];
  info->f_step2 = red[arslam::NPART];
  info->e_step_bad = red[arslam::P_YBAD] != 0.0;
  info->candidate_bad = red[arslam::P_CBAD] != 0.0;
  info->f_step_bad = red[arslam::NPART + 1] != 0.0;
  info->indefinite = red[arslam::NPART + 2] != 0.0;
  // the device vectors by the caller's slots
  std::vector<double> tmp(h->n);
  const struct { const double *src; double *dst; } vecs[5] = {
      {h->d_g.p, g}, {h->d_colnorm.p, colnorm}, {h->d_scale.p, scale}, {h->d_diag.p, diag}, {h->xc, xc}};
  for (const auto &v : vecs) {
    if (!v.dst) continue;
    HIP_CHECK(hipMemcpyAsync(tmp.data(), v.src, h->n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    std::fill(v.dst, v.dst + info->n, 0.0);
    for (long i = 0; i < h->n; ++i)
      if (map[i] >= 0) v.dst[map[i]] = tmp[i];
  }
  if (h->has_f) {
    if (S) HIP_CHECK(hipMemcpyAsync(S, d_dense.p, N * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (y) HIP_CHECK(hipMemcpyAsync(y, h->d_yF.p, h->nR * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    for (long r = 0; r < h->nR && row_slot; ++r) row_slot[r] = rows[r] < 0 ? -1 : (int)map[rows[r]];
  }
}
}  // namespace

extern "C" {

int arslam_lm_debug_step_stages(arslam_lm *h, double radius, arslam_lm_step_info *info, double *g, double *colnorm,
                                double *scale, double *diag, double *S, int *row_slot, double *y, double *xc) {
  if (!h || !info || !(radius > 0.0)) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!h->loaded || h->multi(), ARSLAM_E_STATE, "step_stages: a problem loaded on one rank");
    h->ensure_stream();
    h->cov_invalidate();
    std::memset(info, 0, sizeof(*info));
    const arslam_lm::BlockMap bm = h->block_map();
    std::vector<long> map;
    info->n = caller_slots(h, bm, map);
    info->n_cap = bm.n_cap;
    info->n_tag = bm.n_tag;
    info->elimination_used = h->elim_used;
    info->n_direct = h->elim_used == ARSLAM_ELIM_MIXED ? h->mx.n_direct : 0;
    step_stages(h, radius, false, map, h->lay.row_slot, info, g, colnorm, scale, diag, S, row_slot, y, xc);
  });
}

int arslam_lm_debug_step_stages_sharded(arslam_lm *h, double radius, int lin_exchange, arslam_lm_step_info *info,
                                        int shard[8], double *g, double *colnorm, double *scale, double *diag,
                                        unsigned char *held, double *S, int *row_slot, int *row_class, double *y,
                                        double *xc) {
  if (!h || !info || !shard || !(radius > 0.0) || (lin_exchange != 0 && lin_exchange != 1)) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!h->loaded || !h->multi(), ARSLAM_E_STATE, "step_stages_sharded: a problem loaded on a sharded handle");
    h->ensure_stream();
    h->cov_invalidate();
    std::memset(info, 0, sizeof(*info));
    std::vector<long> map;
    info->n = caller_slots_sharded(h, map);
    info->n_cap = h->nc_full;
    info->n_tag = h->nt;
    info->elimination_used = h->elim_used;
    // the layout's rows (the loaded layout itself is kept on one rank only) and
    // their classes: 0 this rank's subtrees, 1 the replicated top, 2 another rank's
    std::vector<int> rows(h->has_f ? h->nR : 0), cls(rows.size(), 1);
    if (h->has_f) {
      HIP_CHECK(hipMemcpyAsync(rows.data(), h->u_row_slot, rows.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
      HIP_CHECK(hipStreamSynchronize(h->stream));
      for (size_t r = 0; r < rows.size(); ++r) cls[r] = h->plan.h_col_class[r / arslam::kTile];
    }
    std::memset(shard, 0, 8 * sizeof(int));
    shard[0] = h->rank;
    shard[1] = h->nranks;
    shard[2] = h->has_f ? (int)h->plan.n_top_tiles : 0;
    shard[4] = h->nc;
    shard[5] = h->split_active;
    shard[6] = lin_exchange;
    // held: this rank's captures, and an f-side slot unless its row is another
    // rank's (a slot without a row -- a constant or unseen block, or any slot of
    // a problem with no reduced system -- keeps the same bits on every rank)
    std::vector<int> slot_cls(h->n, 1);
    for (size_t r = 0; r < rows.size(); ++r) {
      if (rows[r] < 0) continue;
      slot_cls[rows[r]] = cls[r];
      shard[3] += cls[r] == 1;
    }
    if (held) {
      std::fill(held, held + info->n, (unsigned char)0);
      for (long sl = 0; sl < h->n; ++sl) held[map[sl]] = slot_cls[sl] != 2;
    }
    for (size_t r = 0; r < rows.size() && row_class; ++r) row_class[r] = cls[r];
    step_stages(h, radius, lin_exchange == 1, map, rows, info, g, colnorm, scale, diag, S, row_slot, y, xc);
  });
}

int arslam_lm_add_residual_block(arslam_lm *h, const double corners[8], double *camera,
                                 double *capture, double *tag) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam_lm_add_residual_block_sized(h, corners, camera, capture, tag, h->def_tag_size, h->def_loss_kind,
                                            h->def_loss_a);
}

int arslam_lm_add_residual_block_loss(arslam_lm *h, const double corners[8], double *camera,
                                      double *capture, double *tag, int kind, double a) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam_lm_add_residual_block_sized(h, corners, camera, capture, tag, h->def_tag_size, kind, a);
}

int arslam_lm_add_residual_block_sized(arslam_lm *h, const double corners[8], double *camera,
                                       double *capture, double *tag, double size, int kind, double a) {
  if (!h || !corners || !camera || !capture || !tag) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!arslam::loss_valid(kind, a), ARSLAM_E_INVALID_ARG,
            "loss: kind must be ARSLAM_LOSS_NONE, _HUBER, _SOFT_L_ONE or _CAUCHY, its scale finite and > 0");
    fail_if(!arslam::tag_size_valid(size), ARSLAM_E_INVALID_ARG, "tag size: finite and > 0 (metres)");
    fail_if(h->camera_ptr && h->camera_ptr != camera, ARSLAM_E_UNSUPPORTED,
            "one shared camera block per problem (ArSlamSolver::camera_)");
    fail_if(capture == camera || tag == camera || capture == tag, ARSLAM_E_INVALID_ARG,
            "parameter blocks must be distinct");
    fail_if(h->tag_of.count(capture) || h->cap_of.count(tag), ARSLAM_E_INVALID_ARG,
            "a block cannot be both a capture and a tag");
    h->camera_ptr = camera;
    auto ci = h->cap_of.find(capture);
    int c;
    if (ci == h->cap_of.end()) {
      c = (int)h->cap_ptrs.size();
      h->cap_of.emplace(capture, c);
      h->cap_ptrs.push_back(capture);
    } else {
      c = ci->second;
    }
    auto ti = h->tag_of.find(tag);
    int t;
    if (ti == h->tag_of.end()) {
      t = (int)h->tag_ptrs.size();
      h->tag_of.emplace(tag, t);
      h->tag_ptrs.push_back(tag);
    } else {
      t = ti->second;
    }
    if (ti == h->tag_of.end()) h->pk_appended_only = false;   // a new tag: new reduced rows
    h->eval_drop();
    h->pk_dirty = true;
    h->pk_obs_cap.push_back(c);
    h->pk_obs_tag.push_back(t);
    h->pk_corners.insert(h->pk_corners.end(), corners, corners + 8);
    h->pk_loss_kind.push_back((unsigned char)kind);
    h->pk_loss_a.push_back(kind == ARSLAM_LOSS_NONE ? 0.0 : a);
    h->pk_size.push_back(size);
  });
}

int arslam_lm_set_parameter_block_constant(arslam_lm *h, double *block) {
  if (!h || !block) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(block != h->camera_ptr && !h->cap_of.count(block) && !h->tag_of.count(block),
            ARSLAM_E_INVALID_ARG, "parameter block is not part of the problem");
    if (h->constant.insert(block).second) h->pk_dirty = true, h->pk_appended_only = false, h->eval_drop();
  });
}

int arslam_lm_set_parameter_block_variable(arslam_lm *h, double *block) {
  if (!h || !block) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    if (h->constant.erase(block)) h->pk_dirty = true, h->pk_appended_only = false, h->eval_drop();
  });
}

int arslam_lm_num_residual_blocks(const arslam_lm *h) {
  return h ? (int)h->pk_obs_cap.size() : 0;
}

int arslam_lm_solve(arslam_lm *h, arslam_lm_summary *summary) {
  if (!h || !summary) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    std::memset(summary, 0, sizeof(*summary));
    if (h->pk_obs_cap.empty()) {   // empty problem: nothing to do (Ceres returns immediately)
      summary->termination = ARSLAM_CONVERGENCE;
      return;
    }
    const double t_stage = now_s();
    const int nc = (int)h->cap_ptrs.size(), nt = (int)h->tag_ptrs.size();
    std::vector<double> cam(h->camera_ptr, h->camera_ptr + 3), cap(6L * nc), tag(6L * nt);
    std::vector<unsigned char> cc(nc), tc(nt);
    for (int c = 0; c < nc; ++c) {
      std::memcpy(&cap[6L * c], h->cap_ptrs[c], 6 * sizeof(double));
      cc[c] = h->constant.count(h->cap_ptrs[c]) ? 1 : 0;
    }
    for (int t = 0; t < nt; ++t) {
      std::memcpy(&tag[6L * t], h->tag_ptrs[t], 6 * sizeof(double));
      tc[t] = h->constant.count(h->tag_ptrs[t]) ? 1 : 0;
    }
    arslam_soa_problem p{};
    p.n_cap = nc; p.n_tag = nt; p.n_obs = (int)h->pk_obs_cap.size();
    p.camera = cam.data(); p.cap = cap.data(); p.tag = tag.data();
    p.obs_cap = h->pk_obs_cap.data(); p.obs_tag = h->pk_obs_tag.data();
    p.corners = h->pk_corners.data();
    // (one loss and one tag side per block, beside pk_corners)
    const arslam::ObsLoss pk_loss{h->pk_loss_kind.data(), h->pk_loss_a.data(), h->pk_size.data()};
    p.camera_const = h->constant.count(h->camera_ptr) ? 1 : 0;
    p.cap_const = cc.data(); p.tag_const = tc.data();
    struct StageGuard {   // (the staging arrays go out of scope; the device problem stays)
      arslam_lm *h;
      ~StageGuard() { h->pk_stage = nullptr; h->soa = arslam_soa_problem{}; h->reuse_order = false; }
    } stage_guard{h};
    if (h->loaded && h->pk_loaded && !h->pk_dirty) {
      h->reload_values(&p);   // same problem, new values: no host rebuild, no re-upload of observations
    } else if (h->loaded && h->pk_loaded && h->pk_appended_only && h->try_append(&p, pk_loss)) {
      h->pk_dirty = false;    // appended residual blocks within the loaded tile pattern: layout and plan kept
    } else {
      h->reuse_order = h->pk_loaded;   // a grown pointer-keyed problem (not the first load)
      h->ev_src_set = false;           // (arslam_lm_evaluate: no problem of arslam_lm_load_soa's any more)
      h->load(&p, pk_loss);
      h->reuse_order = false;
      h->pk_loaded = true;
      h->pk_dirty = false;
    }
    if (h->env.setup_profile) std::fprintf(stderr, "arslam stage+setup %.3f ms\n", 1e3 * (now_s() - t_stage));
    h->pk_stage = &p;
    // the final write_back also writes the caller's blocks (Ceres writes parameters back;
    // every iteration under update_state_every_iteration)
    h->solve(summary);
  });
}

int arslam_lm_reset(arslam_lm *h) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    h->camera_ptr = nullptr;
    h->cap_of.clear(); h->tag_of.clear();
    h->cap_ptrs.clear(); h->tag_ptrs.clear();
    h->pk_obs_cap.clear(); h->pk_obs_tag.clear(); h->pk_corners.clear();
    h->pk_loss_kind.clear(); h->pk_loss_a.clear();   // (the default loss stays: it is the handle's, not the problem's)
    h->pk_size.clear();                              // (and so does the default tag side)
    h->constant.clear();
    h->loaded = false;
    h->pk_dirty = true;
    h->eval_drop();
    h->pk_loaded = false;
    h->order.forget();
  });
}

int arslam_lm_load_soa(arslam_lm *h, const arslam_soa_problem *p) {
  return arslam_lm_load_soa_loss(h, p, nullptr, nullptr);
}

int arslam_lm_load_soa_loss(arslam_lm *h, const arslam_soa_problem *p, const unsigned char *obs_loss_kind,
                            const double *obs_loss_a) {
  return arslam_lm_load_soa_sized(h, p, nullptr, obs_loss_kind, obs_loss_a);
}

int arslam_lm_load_soa_sized(arslam_lm *h, const arslam_soa_problem *p, const double *tag_size,
                             const unsigned char *obs_loss_kind, const double *obs_loss_a) {
  if (!h || !p || (obs_loss_kind == nullptr) != (obs_loss_a == nullptr)) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(p->n_obs < 0 || p->n_tag < 0, ARSLAM_E_INVALID_ARG, "negative sizes");   // (before they size anything here)
    if (tag_size) {
      for (int t = 0; t < p->n_tag; ++t)
        fail_if(!arslam::tag_size_valid(tag_size[t]), ARSLAM_E_INVALID_ARG, "tag_size: finite and > 0 (metres)");
      fail_if(p->n_obs > 0 && !p->obs_tag, ARSLAM_E_INVALID_ARG, "null observation arrays");
      for (int b = 0; b < p->n_obs; ++b)
        fail_if(p->obs_tag[b] < 0 || p->obs_tag[b] >= p->n_tag, ARSLAM_E_INVALID_ARG, "obs_tag out of range");
    }
    if (obs_loss_kind)
      for (int b = 0; b < p->n_obs; ++b)
        fail_if(!arslam::loss_valid(obs_loss_kind[b], obs_loss_a[b]), ARSLAM_E_INVALID_ARG,
                "obs_loss: kind must be ARSLAM_LOSS_NONE, _HUBER, _SOFT_L_ONE or _CAUCHY, its scale finite and > 0");
    h->pk_loaded = false;
    h->pk_dirty = true;
    h->reuse_order = false;   // a bulk load never reuses a pointer-keyed problem's order
    h->order.forget();
    // (the caller's arrays are read during the load only)
    arslam::ObsLoss ol = obs_loss_kind ? arslam::ObsLoss{obs_loss_kind, obs_loss_a} : h->default_obs_loss(p->n_obs);
    ol.size = h->obs_sizes(p, tag_size);
    h->ev_src_set = false;
    h->load(p, ol);
    // arslam_lm_evaluate's view of the problem: the caller's arrays (read at the
    // first evaluate), and a copy of the losses that were given for this call only
    h->ev_src = *p;
    h->ev_src_loss_from = obs_loss_kind ? 1 : ol.kind ? 2 : 0;
    h->ev_src_sized = ol.size != nullptr;
    if (obs_loss_kind) {
      h->ev_src_kind.assign(obs_loss_kind, obs_loss_kind + p->n_obs);
      h->ev_src_a.assign(obs_loss_a, obs_loss_a + p->n_obs);
    }
    h->ev_src_set = true;
  });
}

int arslam_lm_solve_loaded(arslam_lm *h, arslam_lm_summary *summary) {
  if (!h || !summary) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(h->pk_loaded, ARSLAM_E_STATE, "no problem loaded by arslam_lm_load_soa");
    h->solve(summary);
  });
}

int arslam_lm_solve_soa(arslam_soa_problem *p, const arslam_lm_options *opt,
                        arslam_lm_summary *summary) {
  if (!p || !summary) return ARSLAM_E_INVALID_ARG;
  arslam_lm *h = nullptr;
  int rc = arslam_lm_create(&h, opt);
  if (rc) return rc;
  rc = arslam::api_guarded([&] {
    h->load(p, arslam::ObsLoss{});   // (a handle of its own: no default loss to apply)
    h->solve(summary);
  });
  arslam_lm_destroy(h);
  return rc;
}

int arslam_lm_debug_reduced_rows(arslam_lm *h, int *cap_row, int *tag_row, int *cam_row) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!h->loaded || h->multi(), ARSLAM_E_STATE, "reduced_rows: a problem loaded on one rank");
    if (cam_row) *cam_row = h->has_f ? h->P.cam_row : -1;
    // a caller's block has a row when it is an f-block (no reduced system: the layout has no rows)
    const arslam_lm::BlockMap bm = h->block_map();
    const auto rows = [&](bool cap, int n, int *row) {
      for (int i = 0; i < n && row; ++i) {
        const int f = bm.role(cap, i) == arslam::kCovF ? bm.idx(cap, i) : -1;
        row[i] = f >= 0 && (size_t)f < h->lay.tag_row.size() ? h->lay.tag_row[f] : -1;
      }
    };
    rows(true, bm.n_cap, cap_row);
    rows(false, bm.n_tag, tag_row);
  });
}

int arslam_comm_unique_id(unsigned char id[ARSLAM_COMM_ID_BYTES]) {
  if (!id) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    static_assert(sizeof(ncclUniqueId) <= ARSLAM_COMM_ID_BYTES, "id size");
    ncclUniqueId u;
    NCCL_CHECK(ncclGetUniqueId(&u));
    std::memset(id, 0, ARSLAM_COMM_ID_BYTES);
    std::memcpy(id, &u, sizeof(u));
  });
}

int arslam_lm_set_comm_callback(arslam_lm *h, int rank, int nranks, arslam_allreduce_fn fn, void *ctx) {
  if (!h || nranks < 1 || rank < 0 || rank >= nranks || ((nranks > 1 || h->force_multi) && !fn))
    return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(h->est_active() && (nranks > 1 || h->force_multi), ARSLAM_E_UNSUPPORTED,
            "estimate_distortion is single-rank only (the l1, l2 rows have no rank exchange)");
    if (h->comm) { (void)ncclCommDestroy(h->comm); h->comm = nullptr; }
    h->rank = rank;
    h->nranks = nranks;
    h->comm_cb = h->multi() ? fn : nullptr;
    h->comm_cb_ctx = ctx;
    h->loaded = false;
    h->pk_dirty = true;
    h->eval_drop();
  });
}

int arslam_lm_set_comm(arslam_lm *h, int rank, int nranks, const unsigned char id[ARSLAM_COMM_ID_BYTES]) {
  if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(h->est_active() && (nranks > 1 || h->force_multi), ARSLAM_E_UNSUPPORTED,
            "estimate_distortion is single-rank only (the l1, l2 rows have no rank exchange)");
    h->ensure_stream();
    if (h->comm) { (void)ncclCommDestroy(h->comm); h->comm = nullptr; }
    h->comm_cb = nullptr;
    h->rank = rank;
    h->nranks = nranks;
    h->loaded = false;
    h->pk_dirty = true;
    h->eval_drop();
    if (h->multi()) {   // (one rank only under arslam_debug_force_multirank)
      ncclUniqueId u;
      std::memcpy(&u, id, sizeof(u));
      NCCL_CHECK(ncclCommInitRank(&h->comm, nranks, u, rank));
    }
  });
}

int arslam_lm_owned_captures(const arslam_lm *h, int *out, int cap, int *n) {
  if (!h || !n || (cap > 0 && !out)) return ARSLAM_E_INVALID_ARG;
  if (!h->loaded) return ARSLAM_E_STATE;
  const int k = h->multi() ? (int)h->own_caps.size() : h->nc_user;   // (one rank: every capture)
  for (int i = 0; i < k && i < cap; ++i) out[i] = h->multi() ? h->own_caps[i] : i;
  *n = k;
  return ARSLAM_OK;
}

int arslam_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int arslam_lm_set_iteration_callback(arslam_lm *h, arslam_iteration_callback fn, void *ctx) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  h->iter_cb = fn;
  h->iter_cb_ctx = ctx;
  return ARSLAM_OK;
}

int arslam_lm_debug_force_indefinite(arslam_lm *h, unsigned long long step_mask) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  h->dbg_indefinite_mask = step_mask;
  return ARSLAM_OK;
}

int arslam_lm_debug_force_multirank(arslam_lm *h, int on) {
  if (!h || (on != 0 && on != 1)) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(on && h->est_active(), ARSLAM_E_UNSUPPORTED,
            "estimate_distortion is single-rank only (the l1, l2 rows have no rank exchange)");
    if (h->comm) { (void)ncclCommDestroy(h->comm); h->comm = nullptr; }
    h->comm_cb = nullptr;
    h->rank = 0;
    h->nranks = 1;
    h->force_multi = on != 0;
    h->loaded = false;
    h->pk_dirty = true;
    h->eval_drop();
  });
}

int arslam_lm_debug_break_dependency(arslam_lm *h, long ticket, long *broken) {
  if (!h || ticket < 0) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!h->loaded || !h->has_f || h->opt.factor_executor != 1, ARSLAM_E_STATE,
            "break_dependency needs a loaded problem on the persistent executor");
    arslam::LltPlan &pl = h->plan;
    long t = ticket;
    while (t < pl.n_dag_tasks && pl.h_dag_wait_off[t] == pl.h_dag_wait_off[t + 1]) ++t;
    fail_if(t >= pl.n_dag_tasks, ARSLAM_E_INVALID_ARG, "no task at or after this ticket waits on anything");
    const int w = pl.h_dag_wait_off[t];
    h->restore_patched_wait();
    pl.h_dag_waits[w].y += 1 << 28;   // a count no task ever reaches (for the next solve only)
    h->dbg_patched_wait = w;
    HIP_CHECK(hipMemcpyAsync(pl.dag_waits + w, &pl.h_dag_waits[w], sizeof(int2), hipMemcpyHostToDevice,
                             h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (broken) *broken = t;
  });
}

int arslam_lm_debug_tag_pair_tile(arslam_lm *h, const double *tag_a, const double *tag_b, int *status) {
  if (!h || !tag_a || !tag_b || !status) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!h->loaded || h->multi() || h->elim_used != ARSLAM_ELIM_CAPTURES || !h->has_f, ARSLAM_E_STATE,
            "tag_pair_tile needs a pointer-keyed problem loaded with capture elimination on one rank");
    const auto ia = h->tag_of.find(const_cast<double *>(tag_a)), ib = h->tag_of.find(const_cast<double *>(tag_b));
    *status = -1;
    if (ia == h->tag_of.end() || ib == h->tag_of.end()) return;
    const int ra = h->lay.tag_row[ia->second], rb = h->lay.tag_row[ib->second];
    if (ra < 0 || rb < 0) return;
    const int T = h->lay.T;
    int st = 2;
    for (int x : {ra, ra + 5})
      for (int y : {rb, rb + 5}) {
        int ti = x / 64, tj = y / 64;
        if (ti < tj) std::swap(ti, tj);
        // (the tiles assembled at the load are numbered first, the fill after them)
        const int id = h->plan.h_tile_id[(size_t)ti * T + tj];
        st = std::min(st, id < 0 ? 0 : (id < h->plan.n_assembled ? 2 : 1));
      }
    *status = st;
  });
}

const char *arslam_lm_last_error(void) { return g_last_error.c_str(); }

#ifndef ARSLAM_BUILD_ID
#define ARSLAM_BUILD_ID "unknown"
#endif
// the build's commit and source digest (ar_slam_amd/build.py build_id): every
// A/B line and bench line names the library it measured
const char *arslam_lm_version(void) { return "arslam_lm 0.2 (gfx950, fp64) build " ARSLAM_BUILD_ID; }

}  // extern "C"
