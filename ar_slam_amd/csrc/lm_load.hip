// lm_load.hip -- the LM handle's problem setup (lm_handle.h): the full load
// (side rule, host structure, elimination order, tile plan, upload), the
// append path that keeps a loaded plan for a grown problem, and the
// values-only reload.
#include "lm_handle.h"

void arslam_lm::check_same_split(const arslam::RankSplit &sp) {
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&](long v) { h = (h ^ (unsigned long long)v) * 1099511628211ull; };
  for (int v : sp.col_owner) mix(v);
  for (int v : sp.cap_owner) mix(v);
  mix(sp.n_active);
  const double hv[2] = {(double)(h >> 12), -(double)(h >> 12)};   // exact in a double
  ensure_stream();
  d_split_hash.alloc(2);
  HIP_CHECK(hipMemcpyAsync(d_split_hash.p, hv, sizeof(hv), hipMemcpyHostToDevice, stream));
  allreduce(d_split_hash.p, 2, ARSLAM_OP_MAX);
  double got[2];
  HIP_CHECK(hipMemcpyAsync(got, d_split_hash.p, sizeof(got), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  fail_if(got[0] != -got[1], ARSLAM_E_COMM,
          "the ranks derived different capture / tile-column splits (same problem and options on every rank, "
          "no rank-dependent ARSLAM_* environment)");
}

void arslam_lm::ensure_stream() {
  int cur = -1;
  HIP_CHECK(hipGetDevice(&cur));
  if (stream && ready_thread == std::this_thread::get_id() && ready_opt_device == opt.device && cur == device) {
    return;
  }
  // the handle's device: the options device, else the one its stream lives on, else the current one
  const int want = opt.device >= 0 ? opt.device : (stream ? device : cur);
  fail_if(stream && want != device, ARSLAM_E_STATE,
          "the handle's device changed after its stream was created (set options.device before the first load)");
  if (want != cur) HIP_CHECK(hipSetDevice(want));   // (set only when it differs)
  device = want;
  if (cus_device != device) {
    cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 0;
    cus_device = device;
    arslam::set_schur_big_lds_attribute();   // (k_schur's big-capture launch: once per device)
  }
  // 1.75 persistent workgroups per CU (73 KB of LDS each: two fit): 448 on
  // the MI355X's 256 CUs.  cfg3 k_factor_dag 663.1 -> 655.7 us and
  // 597.6 -> 593.0 us against 512 (same-box A/B, tools/ab.py): fewer
  // co-resident update workgroups beside the chain's POTRF tasks
  if (cus > 0) dag_workgroups = 7 * cus / 4;
  if (const char *g = std::getenv("ARSLAM_DAG_GRID")) dag_workgroups = std::max(1, std::atoi(g));   // debug
  // never more than can be resident at once (the claim cap is half the grid)
  if (cus > 0) dag_workgroups = std::min(dag_workgroups, arslam::kDagWorkgroupsPerCu * cus);
  if (!stream) HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  for (auto &t : timers) t.init();
  ready_thread = std::this_thread::get_id();
  ready_opt_device = opt.device;
}

// The e-block side (ARSLAM_ELIM_*) for Ceres' set cs of the problem: Ceres' own
// independent set decides AUTO; tag elimination runs the same kernels on the
// role-swapped problem.
int arslam_lm::choose_side(const arslam::SchurSide &cs) {
  ceres_e_cap = cs.e_cap;
  ceres_e_tag = cs.e_tag;
  // (an eliminated block's local system over its distinct f-blocks lives in
  // one wave's LDS: at most kMaxSchurBlocks of them)
  const bool tags_fit = cs.max_tag_blk <= arslam::kMaxSchurBlocks, caps_fit = cs.max_cap_blk <= arslam::kMaxSchurBlocks;
  int side = opt.elimination;
  if (side == ARSLAM_ELIM_AUTO)
    side = (!multi() && tags_fit && (cs.e_tag > cs.e_cap || !caps_fit)) ? ARSLAM_ELIM_TAGS : ARSLAM_ELIM_CAPTURES;
  if (side == ARSLAM_ELIM_MIXED) {
    // Ceres' exact set: a whole side when it holds one kind only (then it is
    // every free block of that kind), the mixed device problem otherwise; the
    // camera joins it only in degenerate graphs (one residual), where the
    // device eliminates the captures instead
    fail_if(multi(), ARSLAM_E_UNSUPPORTED, "the mixed e-block set is single-rank only (the ranks own captures)");
    if (cs.e_cam || cs.e_tag == 0) side = ARSLAM_ELIM_CAPTURES;
    else if (cs.e_cap == 0) side = ARSLAM_ELIM_TAGS;
  }
  fail_if(side == ARSLAM_ELIM_TAGS && multi(), ARSLAM_E_UNSUPPORTED,
          "tag elimination is single-rank only (the ranks own captures)");
  fail_if(multi() && opt.factor_executor != 1, ARSLAM_E_UNSUPPORTED,
          "several ranks need the persistent executor (factor_executor = 1)");
  fail_if(side == ARSLAM_ELIM_TAGS && !tags_fit, ARSLAM_E_UNSUPPORTED,
          "tag elimination: a tag seen by more than 256 distinct captures");
  fail_if(side == ARSLAM_ELIM_CAPTURES && !caps_fit, ARSLAM_E_UNSUPPORTED,
          "capture elimination: a capture sees more than 256 distinct tags");
  return side;
}

// load()'s first stage: the side, and the device problem of that side (p_in
// itself, `swapped`, or the handle's mx).
const arslam_soa_problem *arslam_lm::choose_device_problem(const arslam_soa_problem *p_in, arslam_soa_problem &swapped) {
  std::vector<uint8_t> e_cap, e_tag;
  const bool want_set = opt.elimination == ARSLAM_ELIM_MIXED;
  elim_used = choose_side(arslam::ceres_schur_side(p_in, want_set ? &e_cap : nullptr, want_set ? &e_tag : nullptr));
  return arslam::device_problem(*p_in, elim_used, e_cap, e_tag, swapped, mx);
}

// The tile plan, and on one rank beside it the Schur gather plan (host only,
// from h and L) on a second thread while this one builds and uploads the tile
// plan (its HIP calls stay on the thread whose device is current) and does the
// co-visibility bookkeeping.
void arslam_lm::build_plans(const arslam::HostProblem &h, arslam::ReducedLayout &L, const std::vector<int> &col_class) {
  scalar_flops = L.scalar_flops;
  nR = L.nR;
  has_f = nR > 0;
  sg_ready = false;
  N = has_f ? L.N : 0;
  if (has_f && !multi()) {
    arslam::SchurGather sg_new;
    arslam::host_fork2(
        true, [&] { sg_new = arslam::schur_gather_plan(h, L); },
        [&] {
          arslam::llt_plan_build(plan, L.T, N, L.pattern, stream, nullptr);
          order.graph_build(h, L);
        });
    sg = std::move(sg_new);
    sg_ready = true;
  } else if (has_f) {
    arslam::llt_plan_build(plan, L.T, N, L.pattern, stream, &col_class);
  } else {
    if (!multi()) order.graph_build(h, L);
    arslam::llt_plan_free(plan);
  }
}

// "Estimate the distortion" covers one rank and a whole eliminated side: the
// border of the Schur complement (lm_schur_cam.hip) has no rank exchange and
// no direct groups.  Checked before load() touches the handle.
void arslam_lm::est_check_load(const arslam_soa_problem *p_in) const {
  if (!est_active()) return;
  fail_if(multi(), ARSLAM_E_UNSUPPORTED,
          "estimate_distortion is single-rank only (the l1, l2 rows have no rank exchange)");
  if (opt.elimination != ARSLAM_ELIM_MIXED || !p_in) return;
  const arslam::SchurSide cs = arslam::ceres_schur_side(p_in);
  fail_if(!(cs.e_cam || cs.e_tag == 0 || cs.e_cap == 0), ARSLAM_E_UNSUPPORTED,
          "estimate_distortion: ARSLAM_ELIM_MIXED whose e-block set mixes captures and tags is not supported "
          "(ARSLAM_ELIM_CAPTURES, _TAGS or _AUTO)");
}

void arslam_lm::load(const arslam_soa_problem *p_in, const arslam::ObsLoss &in_loss) {
  const double t_load = now_s();
  est_check_load(p_in);
  loaded = false;
  cov_invalidate();
  eval_drop();
  cov_sp_ready = false;
  cov_tp_ready = false;
  // (the process's first HIP call starts the runtime, 0.02-0.2 s: the first
  // load of a process pays it here, in summary.setup_phase_s[0] -- round 4's
  // "1.2 ms per full load" was that one start averaged over 179 loads)
  ensure_stream();
  arslam_soa_problem swapped;
  const arslam_soa_problem *p = choose_device_problem(p_in, swapped);
  const arslam::MixedProblem *mixed = elim_used == ARSLAM_ELIM_MIXED ? &mx : nullptr;
  arslam::LayoutRequest rq = order.request(reuse_order, elim_used, mixed, opt.reduced_ordering,
                                           opt.cholesky_skip_zero_tiles != 0, p->n_cap);
  const double t_side = now_s();
  double t_host = t_side;   // (one rank: after the host problem)
  arslam::HostProblem h;
  arslam::ReducedLayout L;
  std::vector<int> col_class;
  own_caps.clear();
  nc_full = p->n_cap;
  nc_user = p_in->n_cap;
  if (multi()) {
    local_rank_problem(p, in_loss, rq, h, L, col_class);
  } else {
    h = arslam::device_host_problem(p, mixed, *p_in, &in_loss);
    t_host = now_s();
    rq.fast_order = reuse_order;   // (a grown pointer-keyed problem: a fresh order takes the faster separator search)
    L = order.layout(h, rq);
  }
  const double t_layout = now_s();
  soa = *p;   // (several ranks: the whole problem; write_back maps this rank's captures)
  nc = h.nc;
  nt = h.nt;
  nb = h.nb;
  n = h.n;
  nb_global = h.nb_global;
  slot_free = h.slot_free;
  x0 = h.x0;
  order.remember(L, h, rq, mixed);
  const double t_book = now_s();
  build_plans(h, L, col_class);
  const double t_plan = now_s();
  upload_problem(h, L);
  const double t_upload = now_s();
  if (!multi()) lay = std::move(L);   // (try_append: an appended problem keeps this layout and plan)
  setup_kind = ARSLAM_SETUP_LOAD;
  soa = mixed ? *p_in : *p;   // (mixed: write_back maps the device slots to p_in's blocks)
  loaded = true;
  pk_appended_only = true;
  record_load_times(t_load, t_side, t_host, t_layout, t_book, t_plan, t_upload);
}

// summary.setup_phase_s: structure (side rule + host problem), elimination
// order (reduced layout; several ranks: + the split), tile plan + task graph,
// gather plan + upload, the rest
void arslam_lm::record_load_times(double t_load, double t_side, double t_host, double t_layout, double t_book,
                                  double t_plan, double t_upload) {
  const double t_end = now_s();
  setup_s = t_end - t_load;
  setup_phase[0] = t_host - t_load;
  setup_phase[1] = t_layout - t_host;
  setup_phase[2] = t_plan - t_book;
  setup_phase[3] = t_upload - t_plan;
  setup_phase[4] = setup_s - setup_phase[0] - setup_phase[1] - setup_phase[2] - setup_phase[3];
  if (env.setup_profile)
    std::fprintf(stderr, "arslam setup: nc %d nt %d side %.3f host+layout %.3f covis %.3f plan %.3f gather+upload %.3f tail %.3f total %.3f ms (order %s, %d levels, %ld tiles)\n",
                 nc, nt, 1e3 * (t_side - t_load), 1e3 * (t_layout - t_side), 1e3 * (t_book - t_layout), 1e3 * (t_plan - t_book),
                 1e3 * (t_upload - t_plan), 1e3 * (t_end - t_upload), 1e3 * setup_s,
                 order.last_reused ? "kept" : "fresh", plan.nlev, (long)plan.n_tiles);
}

// Several ranks: every rank holds the whole problem p and computes the same
// structure (deterministic host code, no exchange): the reduced layout, then
// the subtree-to-rank split of the tile elimination tree, which gives this
// rank its captures and tile columns (arslam::rank_split).  h: this rank's
// problem; L: the whole problem's layout, its slots renumbered for this rank.
void arslam_lm::local_rank_problem(const arslam_soa_problem *p, const arslam::ObsLoss &in_loss,
                                   const arslam::LayoutRequest &rq, arslam::HostProblem &h, arslam::ReducedLayout &L,
                                   std::vector<int> &col_class) {
  const arslam::HostProblem hf = arslam::host_problem(p);   // validates p
  L = arslam::reduced_layout(hf, rq);   // (the plain separator search; no recompute for height)
  arslam::RankSplit split = arslam::rank_split(hf, L, std::max(nranks, 2));
  if (nranks == 1) {
    // (forced multi-rank path on one rank: the two-rank split's replicated
    // top, everything below it this rank's -- the exchange then carries the
    // top tiles, as it would between ranks)
    for (int &o : split.col_owner) o = o < 0 ? -1 : 0;
    for (int &o : split.cap_owner) o = 0;
    split.n_active = 1;
  }
  col_class = split.col_class(rank);
  split_top_work = split.top_work;
  split_max_rank_work = split.max_rank_work;
  split_total_work = split.total_work;
  split_active = split.n_active;
  check_same_split(split);
  for (int c = 0; c < p->n_cap; ++c)
    if (split.cap_owner[c] == rank) own_caps.push_back(c);
  // this rank's problem: its captures (ascending), their observations, every tag
  std::vector<int> loc_of(p->n_cap, -1);
  loc_cap.resize(6 * own_caps.size());
  loc_cap_const.assign(own_caps.size(), 0);
  for (size_t c = 0; c < own_caps.size(); ++c) {
    loc_of[own_caps[c]] = (int)c;
    std::memcpy(&loc_cap[6 * c], p->cap + 6L * own_caps[c], 6 * sizeof(double));
    if (p->cap_const) loc_cap_const[c] = p->cap_const[own_caps[c]];
  }
  loc_obs_cap.clear(); loc_obs_tag.clear(); loc_corners.clear();
  loc_loss_kind.clear(); loc_loss_a.clear(); loc_size.clear();
  const bool with_loss = in_loss.kind && in_loss.a;   // (the loss goes with its capture's observations)
  for (int b = 0; b < p->n_obs; ++b) {
    const int lc = loc_of[p->obs_cap[b]];
    if (lc < 0) continue;
    loc_obs_cap.push_back(lc);
    loc_obs_tag.push_back(p->obs_tag[b]);
    loc_corners.insert(loc_corners.end(), p->corners + 8L * b, p->corners + 8L * b + 8);
    if (with_loss) {
      loc_loss_kind.push_back(in_loss.kind[b]);
      loc_loss_a.push_back(in_loss.a[b]);
    }
    if (in_loss.size) loc_size.push_back(in_loss.size[b]);   // (and so does its tag's side)
  }
  const arslam::ObsLoss loc_loss{with_loss ? loc_loss_kind.data() : nullptr, with_loss ? loc_loss_a.data() : nullptr,
                                 in_loss.size ? loc_size.data() : nullptr};
  arslam_soa_problem pl = *p;
  pl.n_cap = (int)own_caps.size();
  pl.n_obs = (int)loc_obs_cap.size();
  pl.cap = loc_cap.data();
  pl.obs_cap = loc_obs_cap.data();
  pl.obs_tag = loc_obs_tag.data();
  pl.corners = loc_corners.data();
  pl.cap_const = p->cap_const ? loc_cap_const.data() : nullptr;
  h = arslam::host_problem(&pl, &loc_loss, p);   // (the tags' use and the observation count: the whole problem's)
  // the layout's tag slots are the whole problem's (3 + 6 nc_full + 6 t + a):
  // renumber them for this rank's parameter vector (3 + 6 nc_own + 6 t + a)
  const long shift = 6L * (p->n_cap - (long)own_caps.size());
  for (int &sl : L.row_slot)
    if (sl >= 3) sl -= (int)shift;
}

// Everything the device needs from the host structure, the layout and the
// Schur gather plan, in one upload (UploadArena), plus the scratch buffers
// sized for the problem.  Ends with the load's one stream sync.
void arslam_lm::upload_problem(const arslam::HostProblem &h, const arslam::ReducedLayout &L, int extend_from) {
  const int maxk = h.maxk;
  cov_invalidate();   // (an appended problem too: its last solve was another problem's)
  const std::vector<int> &row_slot = L.row_slot;
  // f-side slot -> reduced row (camera slots 0..2, then the tag slots)
  std::vector<int> fslot_row(3 + 6L * nt, -1);
  for (size_t r = 0; r < row_slot.size(); ++r) {
    const long sl = row_slot[r];
    if (sl < 0) continue;
    if (sl < 3) fslot_row[sl] = (int)r;
    else if (sl >= 3 + 6L * nc) fslot_row[sl - 6L * nc] = (int)r;
  }
  const bool prof = env.setup_profile;
  const double tu0 = prof ? now_s() : 0.0;
  if (!has_f) sg = arslam::SchurGather{};
  else if (sg_ready) {}   // (load: built beside the tile plan)
  else if (extend_from >= 0 && (int)sg.cap_off.size() == extend_from + 1) arslam::schur_gather_extend(sg, h, L, extend_from);
  else sg = arslam::schur_gather_plan(h, L);
  sg_ready = false;
  const double tu1 = prof ? now_s() : 0.0;
  const int n_dest = has_f ? (int)sg.dest_start.size() - 1 : 0;
  const int n_items = (int)sg.items.size() / 4, n_splits = (int)sg.splits.size() / 4;
  upload.add(&u_cap_start, h.cap_start.data(), nc + 1);
  upload.add(&u_obs_tag, h.obs_tag.data(), nb);
  upload.add(&u_obs_lblk, h.obs_lblk.data(), nb);
  upload.add(&u_cap_blk_start, h.cap_blk_start.data(), nc + 1);
  upload.add(&u_blk_tag, h.blk_tag.data(), h.blk_tag.size());
  upload.add(&u_tag_start, h.tag_start.data(), nt + 1);
  upload.add(&u_obs_tpos, h.obs_tpos.data(), nb);
  upload.add(&u_obs_active, h.obs_active.data(), nb);
  upload.add(&u_slot_free, h.slot_free.data(), n);
  upload.add(&u_corners, h.corners.data(), 8L * nb);
  const bool has_loss = !h.loss_kind.empty();   // (permuted with the corners by host_problem)
  if (has_loss) {
    upload.add(&u_loss_kind, h.loss_kind.data(), nb);
    upload.add(&u_loss_a, h.loss_a.data(), nb);
  }
  const bool has_size = !h.obs_size.empty();
  if (has_size) upload.add(&u_obs_size, h.obs_size.data(), nb);
  upload.add(&u_x0, x0.data(), n);
  upload.add(&u_tag_row, L.tag_row.data(), L.tag_row.size());
  upload.add(&u_row_slot, row_slot.data(), row_slot.size());
  upload.add(&u_fslot_row, fslot_row.data(), fslot_row.size());
  // several ranks: the top tags' slots (their linearization sums ride with the top tiles)
  std::vector<int> top_slots;
  if (multi() && has_f)
    for (long sl = 3 + 6L * nc; sl < n; ++sl) {
      const int r = fslot_row[sl - 6L * nc];
      if (r >= 0 && plan.h_col_class[r / arslam::kTile] == 1) top_slots.push_back((int)sl);
    }
  n_top_slots = (int)top_slots.size();
  if (n_top_slots) upload.add(&u_top_slots, top_slots.data(), top_slots.size());
  // several ranks: the f-side slots this rank holds -- its own subtree's tag
  // rows; the top's rows, the camera and the tags outside the reduced system
  // on rank 0 (every rank holds the top, one counts it); capture slots all
  f_own.clear();
  if (multi()) {
    f_own.assign(n, 0);
    for (long sl = 3; sl < 3 + 6L * nc; ++sl) f_own[sl] = 1;
    for (long sl = 0; sl < n; ++sl) {
      if (sl >= 3 && sl < 3 + 6L * nc) continue;
      const int r = fslot_row[sl < 3 ? sl : sl - 6L * nc];
      const int cls = r >= 0 && has_f ? plan.h_col_class[r / arslam::kTile] : 1;
      f_own[sl] = cls == 0 || (cls == 1 && rank == 0);
    }
    upload.add(&u_f_own, f_own.data(), f_own.size());
  }
  const bool mixed = elim_used == ARSLAM_ELIM_MIXED;
  if (mixed) {
    // the direct groups' slots copy f-block slots: counted once, on the f-block
    f_own.assign(n, 1);
    for (int g = 0; g < nc; ++g)
      if (mx.kind[g] == arslam::kMixDirect) std::fill(f_own.begin() + 3 + 6L * g, f_own.begin() + 9 + 6L * g, 0);
    upload.add(&u_f_own, f_own.data(), f_own.size());
    upload.add(&u_cap_kind, mx.kind.data(), mx.kind.size());
    upload.add(&u_f_alias, mx.f_alias.data(), mx.f_alias.size());
  }
  big_caps.clear();
  for (int c = 0; c < nc; ++c)
    if (h.cap_blk_start[c + 1] - h.cap_blk_start[c] > arslam::kSchurMfmaBlocks) big_caps.push_back(c);
  if (!big_caps.empty()) upload.add(&u_big_caps, big_caps.data(), big_caps.size());
  chunk_caps.clear();
  for (int c = 0; c < nc; ++c)
    if (h.cap_start[c + 1] - h.cap_start[c] > arslam::kObsChunk) chunk_caps.push_back(c);
  if (!chunk_caps.empty()) upload.add(&u_chunk_caps, chunk_caps.data(), chunk_caps.size());
  if (has_f) {
    upload.add(&u_cap_off, sg.cap_off.data(), nc + 1);
    upload.add(&u_dest_row, reinterpret_cast<const int2 *>(sg.dest_row.data()), n_dest);
    upload.add(&u_dest_start, sg.dest_start.data(), n_dest + 1);
    upload.add(&u_contrib, sg.contrib.data(), sg.contrib.size());
    upload.add(&u_gather_items, reinterpret_cast<const int4 *>(sg.items.data()), n_items);
    upload.add(&u_gather_splits, reinterpret_cast<const int4 *>(sg.splits.data()), n_splits);
  }
  // l1, l2 estimated (est_check_load passed: one rank, a whole side): per
  // f-block the (e-block, local block) pairs that see it, in e-block order
  const bool est = est_active() && has_f && L.cam_row >= 0;
  if (est) {
    camg_start.assign(nt + 1, 0);
    for (int t : h.blk_tag) camg_start[t + 1]++;
    for (int t = 0; t < nt; ++t) camg_start[t + 1] += camg_start[t];
    camg_items.assign(2 * h.blk_tag.size(), 0);
    std::vector<int> fill(camg_start.begin(), camg_start.end() - 1);
    for (int c = 0; c < nc; ++c)
      for (int a = h.cap_blk_start[c]; a < h.cap_blk_start[c + 1]; ++a) {
        const int at = fill[h.blk_tag[a]]++;
        camg_items[2L * at] = c;
        camg_items[2L * at + 1] = a - h.cap_blk_start[c];
      }
    upload.add(&u_camg_start, camg_start.data(), camg_start.size());
    upload.add(&u_camg_items, reinterpret_cast<const int2 *>(camg_items.data()), camg_items.size() / 2);
  }
  n_clear = has_f ? plan.n_tiles : 0;
  if (has_f && !multi()) {
    // does the gather write into a fill tile (an appended problem's new
    // coupling; the plan is kept)?
    const int T = plan.T;
    bool fill_gathered = false;
    for (int d = 0; d < n_dest && !fill_gathered; ++d) {
      const int rX = sg.dest_row[2L * d], rY = sg.dest_row[2L * d + 1];
      const int sx = (rX == nR || rX == L.cam_row) ? 1 : 6, sy = rY == L.cam_row ? 1 : 6;
      for (int I = rX >> 6; I <= (rX + sx - 1) >> 6; ++I)
        for (int J = rY >> 6; J <= (rY + sy - 1) >> 6 && J <= I; ++J)
          fill_gathered = fill_gathered || plan.h_tile_id[(long)I * T + J] >= plan.n_assembled;
    }
    if (!fill_gathered && plan.fill_first_ok) n_clear = plan.n_assembled;
  }
  upload.commit(stream);
  alloc_solve_buffers();

  P.nc = nc; P.nt = nt; P.nb = nb; P.n = n; P.nR = nR; P.N = N; P.lda = N; P.cam_row = L.cam_row;
  P.max_obs_per_cap = std::max(maxk, 1);
  P.max_blk_per_cap = h.maxblk;
  P.big_caps = big_caps.empty() ? nullptr : u_big_caps;
  P.n_big_caps = (int)big_caps.size();
  P.chunk_caps = chunk_caps.empty() ? nullptr : u_chunk_caps;
  P.n_chunk_caps = (int)chunk_caps.size();
  P.swap_roles = elim_used == ARSLAM_ELIM_TAGS ? 1 : 0;
  P.nf = 3 + 6 * nt;
  P.fslot_row = u_fslot_row;
  P.cap_start = u_cap_start; P.obs_tag = u_obs_tag; P.obs_lblk = u_obs_lblk;
  P.cap_blk_start = u_cap_blk_start; P.blk_tag = u_blk_tag;
  P.obs_active = u_obs_active; P.slot_free = u_slot_free;
  P.tag_start = u_tag_start; P.obs_tpos = u_obs_tpos; P.corners = u_corners;
  P.obs_loss_kind = has_loss ? u_loss_kind : nullptr;
  P.obs_loss_a = has_loss ? u_loss_a : nullptr;
  P.obs_size = has_size ? u_obs_size : nullptr;
  P.camera_radial = camera_model == ARSLAM_CAMERA_RADIAL ? 1 : 0;   // (the handle's model, bound at the load)
  if (est) {   // (allocated under the switch only)
    d_jrows_l.alloc(std::max(16L * nb, 1L));
    d_cam_slab.alloc(std::max(8L * nc + 12L * (long)h.blk_tag.size(), 1L));
    d_lparts.alloc(4L * std::max(nc, 1));
    d_lred.alloc(4);
  }
  est_loaded = est;
  CL = arslam::DevCamL{};
  if (est) {
    CL.jrows_l = d_jrows_l.p;
    CL.lparts = d_lparts.p;
    CL.lred = d_lred.p;
    CL.cam_slab = d_cam_slab.p;
    CL.camg_start = u_camg_start;
    CL.camg_items = u_camg_items;
  }
  P.tag_row = u_tag_row; P.row_slot = u_row_slot;
  P.tile_id = plan.tile_id; P.T = plan.T;
  P.tile_class = multi() && has_f ? plan.tile_class : nullptr;
  P.f_own = multi() || mixed ? u_f_own : nullptr;
  P.cap_kind = mixed ? u_cap_kind : nullptr;
  P.f_alias = mixed ? u_f_alias : nullptr;
  P.cap_off = u_cap_off; P.slab = d_slab.p; P.dest_row = u_dest_row; P.dest_start = u_dest_start;
  P.contrib = u_contrib; P.n_dest = n_dest; P.jrows = d_jrows.p; P.cap_ui = d_cap_ui.p;
  P.gather_items = u_gather_items; P.gather_splits = u_gather_splits; P.gather_part = d_gather_part.p;
  P.n_items = n_items; P.n_splits = n_splits;
  const double tu2 = prof ? now_s() : 0.0;
  // (no sync: the copy reads the arena's page-locked image, which stays
  // untouched until the next upload -- after this solve's syncs)
  if (prof)
    std::fprintf(stderr, "arslam upload: gather plan %.3f arena+allocs %.3f sync %.3f ms\n", 1e3 * (tu1 - tu0),
                 1e3 * (tu2 - tu1), 1e3 * (now_s() - tu2));
}

// the parameter vectors and a step's scratch, sized for the loaded problem
// (grow-only); Sp and d_norms_p point into them
void arslam_lm::alloc_solve_buffers() {
  d_xa.alloc(n); d_xb.alloc(n); d_xbest.alloc(n);
  d_g.alloc(n); d_colnorm.alloc(n); d_scale.alloc(n); d_diag.alloc(n);
  d_obs_tg.alloc(std::max(12L * nb, 1L));
  d_jrows.alloc(std::max(8L * arslam::kJStored * nb, 1L));
  d_cap_ui.alloc(std::max(36L * nc, 1L));
  d_parts.alloc((size_t)arslam::NPART * std::max(nc, 1));
  n_fparts = (int)((std::max(nR, 1L) + 255) / 256);
  d_fparts.alloc(2L * std::max(n_fparts, 1));
  // stays zero when there are no reduced rows (k_update_f is then not launched)
  if (!has_f) HIP_CHECK(hipMemsetAsync(d_fparts.p, 0, d_fparts.n * sizeof(double), stream));
  const double *red_prev = d_red.p;
  d_red.alloc(kLinSave + 8);   // LM scalars | slot norms: results, block count, k_slot_norms block partials | saved
  d_norms_p = d_red.p + 16;       // (one D2H carries both after a linearization)
  if (d_red.p != red_prev) HIP_CHECK(hipMemsetAsync(d_norms_p + 7, 0, sizeof(double), stream));   // the count
  d_flag.alloc(1);
  const int *seq_prev = d_seq_done.p;
  d_seq_done.alloc(1);
  if (d_seq_done.p != seq_prev) HIP_CHECK(hipMemsetAsync(d_seq_done.p, 0, sizeof(int), stream));
  if (has_f) {
    d_slab.alloc(std::max(sg.cap_off[nc], 1L));
    d_gather_part.alloc(36L * std::max(sg.n_pslots, 1));
    s_pre = multi() ? arslam::round_up(top_tail_len(), 512) : 0;
    d_S.alloc((size_t)s_pre + (size_t)plan.n_tiles * 4096);   // (cleared by k_schur's extra blocks every step)
    Sp = d_S.p + s_pre;
    d_z.alloc(N);
    d_yF.alloc(N);
  } else {
    d_S.release();
    Sp = nullptr;
    s_pre = 0;
    d_z.release();
    d_yF.alloc(1);
  }
  HIP_CHECK(hipMemsetAsync(d_parts.p, 0, d_parts.n * sizeof(double), stream));
}

// ---- the append path ----
//
// An appended problem (arslam_lm_solve after AddResidualBlock only, no new
// tag, no constant changed): if every touched group's tile pairs are tiles of
// the loaded factor (assembled or fill: k_schur clears every tile of S each
// step and the gather addresses any of them), the reduced layout, the
// elimination order and the whole factorization plan stay as they are -- only
// the eliminated side, the gather plan and the values are rebuilt and
// uploaded.  false: load() instead, and the handle is as it was but for the
// co-visibility graph and AUTO's ceres_e_*, which that load rebuilds.
// (summary.factor_scalar_flops keeps the loaded problem's count: a new
// coupling inside a fill tile changes the scalar structure.)  A front end per
// eliminated side builds the device problem; the checks and the commit are shared.

// Captures eliminated: p as it is.  (ARSLAM_ELIM_MIXED whose set was every
// capture: new captures join it, as in append_as_mixed.)
bool arslam_lm::append_as_captures(const arslam_soa_problem *p) {
  if (elim_used != ARSLAM_ELIM_CAPTURES ||
      (opt.elimination != ARSLAM_ELIM_AUTO && opt.elimination != ARSLAM_ELIM_CAPTURES &&
       opt.elimination != ARSLAM_ELIM_MIXED))
    return false;
  if (opt.elimination == ARSLAM_ELIM_AUTO) {   // the side Ceres would eliminate may change as the graph grows
    const arslam::SchurSide cs = arslam::ceres_schur_side(p);
    if (cs.max_tag_blk <= arslam::kMaxSchurBlocks && (cs.e_tag > cs.e_cap || cs.max_cap_blk > arslam::kMaxSchurBlocks))
      return false;
    ceres_e_cap = cs.e_cap;
    ceres_e_tag = cs.e_tag;
  }
  return p->n_tag == nt;
}

// ARSLAM_ELIM_MIXED on a grown pointer-keyed problem (the reference's
// solveIncremental, ar_slam_util.cpp:629-742: new captures, each with
// residual blocks of known tags).  A fresh load would recompute Ceres' set
// (ComputeStableSchurOrdering) and rebuild the layout, plan and gather plan;
// here the set only grows: every new capture whose tags are all on the
// reduced side joins it as an eliminated group, appended after the loaded
// groups (so the loaded groups, the f-blocks and the gather plan's summation
// order are kept, and the plan is extended as for captures), and tags never
// leave the reduced side -- a new capture that sees an eliminated tag, a new
// tag or a residual on an old capture reloads.  The set is then the loaded
// problem's Ceres set plus the new captures: an independent set (a new
// capture is adjacent only to its tags, all reduced), not necessarily the
// one Ceres would pick on the grown graph; the step is the same exact solve.
// m: mx grown by the new groups, with p's values (m.soa is the device problem).
bool arslam_lm::append_as_mixed(const arslam_soa_problem *p, arslam::MixedProblem &m) {
  if (elim_used != ARSLAM_ELIM_MIXED || opt.elimination != ARSLAM_ELIM_MIXED) return false;
  const long nb_old = (long)mx.obs_cap.size();
  const int nf = (int)mx.f_src.size();
  if (p->n_tag != mx.src_n_tag || p->n_cap < mx.src_n_cap || p->n_obs <= nb_old) return false;
  // the f-block of each original tag (-1: eliminated or not a parameter)
  std::vector<int> tag_f(p->n_tag, -1);
  for (int f = 0; f < nf; ++f)
    if (!mx.f_is_cap[f]) tag_f[mx.f_src[f]] = f;
  // the new residuals: on new captures only, every tag on the reduced side
  for (long b = nb_old; b < p->n_obs; ++b)
    if (p->obs_cap[b] < mx.src_n_cap || tag_f[p->obs_tag[b]] < 0) return false;
  m = mx;
  const int nc_new = p->n_cap - mx.src_n_cap;
  std::vector<int> cap_g(nc_new, -1);
  for (long b = nb_old; b < p->n_obs; ++b) {
    const int c = p->obs_cap[b], q = c - mx.src_n_cap;
    if (cap_g[q] < 0) {
      cap_g[q] = (int)m.kind.size();
      m.kind.push_back(arslam::kMixCap);
      m.group_src.push_back(c);
      m.cap_const.push_back(p->cap_const ? p->cap_const[c] : 0);
    }
    m.obs_cap.push_back(cap_g[q]);
    m.obs_tag.push_back(tag_f[p->obs_tag[b]]);
  }
  for (int q = 0; q < nc_new; ++q)
    if (cap_g[q] < 0) return false;   // (a capture without residual blocks: not a block of Ceres' problem)
  const int ng = (int)m.kind.size();
  m.src_n_cap = p->n_cap;
  m.cap.resize(6L * ng);
  m.soa = *p;
  m.soa.n_cap = ng;
  m.soa.n_tag = nf;
  m.soa.cap = m.cap.data();
  m.soa.tag = m.tag.data();
  m.soa.obs_cap = m.obs_cap.data();
  m.soa.obs_tag = m.obs_tag.data();
  m.soa.cap_const = m.cap_const.data();
  m.soa.tag_const = m.tag_const.data();
  std::vector<double> xv(3 + 6L * ng + 6L * nf);
  arslam::mixed_values(m, *p, xv.data());
  std::memcpy(m.cap.data(), xv.data() + 3, 6L * ng * sizeof(double));
  if (nf) std::memcpy(m.tag.data(), xv.data() + 3 + 6L * ng, 6L * nf * sizeof(double));
  return true;
}

// the same free f-blocks and camera as the loaded layout (the same reduced rows)
bool arslam_lm::same_reduced_rows(const arslam::HostProblem &h) const {
  if ((lay.cam_row >= 0) != (h.slot_free[0] != 0)) return false;
  for (int t = 0; t < nt; ++t)
    if ((lay.tag_row[t] >= 0) != (h.slot_free[3 + 6L * h.nc + 6L * t] != 0)) return false;
  return true;
}

// every group's tiles pairwise in the loaded factor's tiles (lay.pattern is the
// filled pattern: llt_plan_build fills it in place; a new coupling in a fill
// tile is gathered into it -- k_schur clears every tile of the factor each
// step and the updates read-modify-write their targets)
bool arslam_lm::groups_fit_plan(const arslam::HostProblem &h, const std::vector<int> &groups) const {
  const int T = lay.T;
  std::vector<int> ts;
  for (int c : groups) {
    ts.clear();
    arslam::group_tiles(h, lay.tag_row, lay.cam_row, c, ts);
    for (size_t a = 0; a < ts.size(); ++a)
      for (size_t b = 0; b < ts.size(); ++b)
        if (ts[a] >= ts[b] && plan.h_tile_id[(size_t)ts[a] * T + ts[b]] < 0) return false;
  }
  return true;
}

// arslam_lm_solve's one append entry: the capture form first, then the mixed
// one.  An appended ARSLAM_ELIM_MIXED problem keeps the loaded side's
// ceres_e_* plus the new captures (they are not re-derived on the grown graph).
bool arslam_lm::try_append(const arslam_soa_problem *p, const arslam::ObsLoss &in_loss) {
  if (!loaded || multi() || !has_f) return false;
  if (est_active()) return false;   // (the border's gather lists are built by a full load)
  const double t0 = now_s();
  arslam::MixedProblem m;
  const arslam_soa_problem *dev = nullptr;   // the device problem's source
  if (append_as_captures(p)) dev = p;
  else if (append_as_mixed(p, m)) dev = &m.soa;
  else return false;
  const bool mixed = dev != p;
  const double t1 = now_s();
  const arslam::HostProblem h = arslam::device_host_problem(dev, mixed ? &m : nullptr, *p, &in_loss);
  const double t2 = now_s();
  // the groups to check, ascending: the captures of the appended residual
  // blocks (the others' tile pairs were in the pattern already); mixed: the
  // new groups [nc, h.nc)
  std::vector<char> touched(h.nc, 0);
  for (long b = nb; b < p->n_obs; ++b) touched[mixed ? m.obs_cap[b] : p->obs_cap[b]] = 1;
  std::vector<int> groups;
  for (int c = 0; c < h.nc; ++c)
    if (touched[c]) groups.push_back(c);
  if (!same_reduced_rows(h) || !groups_fit_plan(h, groups)) return false;
  // the order's graph outgrown, or a quarter more groups: reload with a fresh order
  order.add_groups(h, lay, groups);
  if (order.outgrown(h.nc)) return false;
  // only new groups got residual blocks: their contributions extend the gather plan
  const int extend_from = groups.empty() || groups.front() >= nc ? nc : -1;
  // the f-side slots move with the group count
  for (int &sl : lay.row_slot)
    if (sl >= 3) sl += 6 * (h.nc - nc);
  if (mixed) {
    ceres_e_cap += p->n_cap - mx.src_n_cap;
    mx = std::move(m);   // (the moved vectors keep their buffers: mx.soa's pointers stay valid)
  }
  nc = h.nc;
  nc_full = h.nc;   // (reload_values checks the next unchanged solve against it)
  nc_user = p->n_cap;
  nb = h.nb;
  n = h.n;
  nb_global = h.nb_global;
  slot_free = h.slot_free;
  x0 = h.x0;
  const double t3 = now_s();
  upload_problem(h, lay, extend_from);
  soa = *p;
  pk_appended_only = true;
  setup_kind = ARSLAM_SETUP_APPEND;
  setup_s = now_s() - t0;
  if (env.setup_profile)
    std::fprintf(stderr, "arslam append: nc %d side %.3f host %.3f check %.3f upload %.3f ms\n", nc,
                 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (now_s() - t3));
  return true;
}

// Same structure as the loaded problem, new parameter values (the pointer-keyed
// path when no block, residual or constant changed since the last load).
void arslam_lm::reload_values(const arslam_soa_problem *p_in) {
  const double t0 = now_s();
  const arslam_soa_problem swapped = arslam::swap_roles(*p_in);
  const arslam_soa_problem *p = elim_used == ARSLAM_ELIM_TAGS ? &swapped : p_in;
  if (elim_used == ARSLAM_ELIM_MIXED) {   // the regrouped slots from p_in's blocks
    fail_if(!loaded || p_in->n_obs != (int)mx.obs_cap.size() || p_in->n_cap != mx.src_n_cap ||
                p_in->n_tag != mx.src_n_tag, ARSLAM_E_STATE,
            "reload_values: structure differs from the loaded problem");
    arslam::mixed_values(mx, *p_in, x0.data());
  } else {
    fail_if(!loaded || p->n_cap != nc_full || p->n_tag != nt || (!multi() && p->n_obs != nb), ARSLAM_E_STATE,
            "reload_values: structure differs from the loaded problem");
    std::memcpy(x0.data(), p->camera, 3 * sizeof(double));
    if (multi()) {
      for (int c = 0; c < nc; ++c) std::memcpy(x0.data() + 3 + 6L * c, p->cap + 6L * own_caps[c], 6 * sizeof(double));
    } else if (nc) {
      std::memcpy(x0.data() + 3, p->cap, 6L * nc * sizeof(double));
    }
    if (nt) std::memcpy(x0.data() + 3 + 6L * nc, p->tag, 6L * nt * sizeof(double));
  }
  HIP_CHECK(hipMemcpyAsync(u_x0, x0.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  soa = *p;
  setup_kind = ARSLAM_SETUP_VALUES;
  setup_s = now_s() - t0;
}
