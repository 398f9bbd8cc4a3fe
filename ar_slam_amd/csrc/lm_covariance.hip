// lm_covariance.hip -- arslam_lm_covariance and arslam_lm_covariance_pairs on the LM handle (lm_handle.h),
// their _lens forms and their _anchored forms (a pose block held fixed for the call; any e-block set).
#include "lm_handle.h"

#include <map>

void arslam_lm::cov_check_state(const char *who, bool lens, bool anchored) const {
  const std::string w(who);
  fail_if(!lens && est_active(), ARSLAM_E_UNSUPPORTED,
          w + ": not supported while estimate_distortion is on (its camera output is one scalar: use the _lens form)");
  fail_if(!loaded || solve_state == 0, ARSLAM_E_STATE, w + ": no completed solve of the loaded problem");
  fail_if(solve_state == 2, ARSLAM_E_STATE, w + ": the last solve ended with rule EVAL_FAILED");
  fail_if(multi(), ARSLAM_E_UNSUPPORTED, w + ": single-rank only");
  fail_if(!anchored && elim_used == ARSLAM_ELIM_MIXED, ARSLAM_E_UNSUPPORTED,
          w + ": the mixed e-block set is not supported (ARSLAM_ELIM_CAPTURES or _TAGS, or the _anchored form)");
}

arslam_lm::CovRoles arslam_lm::cov_roles() const {
  CovRoles ro;
  const auto size = [&](int n_cap, int n_tag) {
    ro.n_cap = n_cap;
    ro.n_tag = n_tag;
    ro.cap_role.assign(n_cap, arslam::kCovF);
    ro.cap_idx.assign(n_cap, -1);
    ro.tag_role.assign(n_tag, arslam::kCovF);
    ro.tag_idx.assign(n_tag, -1);
    ro.e_node.assign(nc, -1);
    ro.f_node.assign(nt, -1);
  };
  const auto put = [&](bool cap, int i, int role, int idx) {
    (cap ? ro.cap_role : ro.tag_role)[i] = role;
    (cap ? ro.cap_idx : ro.tag_idx)[i] = idx;
    (role == arslam::kCovE ? ro.e_node : ro.f_node)[idx] = cap ? i : ro.n_cap + i;
  };
  if (elim_used == ARSLAM_ELIM_MIXED) {
    size(mx.src_n_cap, mx.src_n_tag);
    for (int f = 0; f < nt; ++f) put(mx.f_is_cap[f] != 0, mx.f_src[f], arslam::kCovF, f);
    for (int g = 0; g < nc; ++g) {
      if (mx.kind[g] == arslam::kMixDirect) ro.e_node[g] = mx.group_src[g];   // (its capture: an f-block)
      else put(mx.kind[g] == arslam::kMixCap, mx.group_src[g], arslam::kCovE, g);
    }
  } else if (elim_used == ARSLAM_ELIM_TAGS) {   // e-blocks: the tags, f-blocks: the captures
    size(nt, nc);
    for (int t = 0; t < nc; ++t) put(false, t, arslam::kCovE, t);
    for (int c = 0; c < nt; ++c) put(true, c, arslam::kCovF, c);
  } else {
    size(nc, nt);
    for (int c = 0; c < nc; ++c) put(true, c, arslam::kCovE, c);
    for (int t = 0; t < nt; ++t) put(false, t, arslam::kCovF, t);
  }
  return ro;
}

void arslam_lm::cov_check_anchor(const char *who, const CovAnchor &an, const CovRoles &ro) const {
  const std::string w(who);
  fail_if(an.kind != ARSLAM_BLOCK_NONE && an.kind != ARSLAM_BLOCK_CAPTURE && an.kind != ARSLAM_BLOCK_TAG,
          ARSLAM_E_INVALID_ARG, w + ": the anchor's kind must be ARSLAM_BLOCK_CAPTURE, _TAG or _NONE");
  if (an.none()) return;
  const int nblk = an.kind == ARSLAM_BLOCK_CAPTURE ? ro.n_cap : ro.n_tag;
  fail_if(an.index < 0 || an.index >= nblk, ARSLAM_E_INVALID_ARG, w + ": the anchor's index is out of range");
}

// The structural gauge check on the host, then one linearization at the point
// the last solve returned, the reduced system without the LM diagonal (its own
// elimination kernel, the LM step's gather) and its factorization as in an LM
// step.  Everything it writes on the device is scratch the next solve rebuilds
// from the loaded state.  lens (the _lens entry points) on a problem whose l1, l2
// are live: they are rows of H like f -- k_cov_schur_cam's border and the LM
// step's border gather put them into the reduced system (cov_lens.hip).
// assemble_only (arslam_lm_debug_cov_camera_rows): stop before the factorization.
//
// an (the _anchored entry points): the call's anchor is held fixed without an
// elimination of its own.  Every covariance kernel reads a copy of the Jacobi
// scale with 0 on the anchor's six slots: an anchored e-block takes the
// constant e-block's path (Q = 0, G = 0), an anchored f-block's columns vanish
// and the gather's diagonal 1 makes its rows decoupled identity rows; the
// callers override the anchor's outputs.  Under a mixed e-block set the copy
// is 0 on the direct groups' slots too -- k_cov_schur then leaves them no Q, G
// or R -- and k_cov_direct stores their local systems (cov_direct.hip).
void arslam_lm::cov_factor(CovFactor &cf, bool lens, bool assemble_only, const CovAnchor *an) {
  ensure_stream();
  cf.live = lens && est_loaded;
  cf.roles = cov_roles();
  cf.scale = d_scale.p;
  const CovRoles &ro = cf.roles;
  if (an && !an->none()) {
    const bool cap = an->kind == ARSLAM_BLOCK_CAPTURE;
    cf.anchor_role = ro.role(cap, an->index);
    cf.anchor_idx = ro.idx(cap, an->index);
    cf.anchor_slot = cf.anchor_role == arslam::kCovE ? 3 + 6L * cf.anchor_idx : 3 + 6L * nc + 6L * cf.anchor_idx;
  }
  std::vector<double> h_scale(an ? n : 0);
  if (an) HIP_CHECK(hipMemcpyAsync(h_scale.data(), d_scale.p, n * sizeof(double), hipMemcpyDeviceToHost, stream));
  // the device problem's structure (its host copy is not kept after a load)
  std::vector<int> &h_cs = cf.cap_start;
  h_cs.assign(nc + 1, 0);
  std::vector<int> h_ot(std::max(nb, 1));
  std::vector<unsigned char> h_act(std::max(nb, 1));
  int n_blk = 0;
  HIP_CHECK(hipMemcpyAsync(h_cs.data(), u_cap_start, (nc + 1) * sizeof(int), hipMemcpyDeviceToHost, stream));
  if (nb) HIP_CHECK(hipMemcpyAsync(h_ot.data(), u_obs_tag, nb * sizeof(int), hipMemcpyDeviceToHost, stream));
  if (nb) HIP_CHECK(hipMemcpyAsync(h_act.data(), u_obs_active, nb, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(&n_blk, u_cap_blk_start + nc, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  // Gauge: every connected component of the caller's capture / tag graph over
  // the active observations that holds a free block must hold a constant one
  // (the call's anchor counts as constant).  An observation joins the caller's
  // blocks of its group and its f-block (CovRoles: a direct group's is its
  // capture, no block of its own), so the outcome does not depend on the
  // e-block set.
  bool deficient = false;
  {
    const int nn = ro.n_cap + ro.n_tag;
    std::vector<int> par(nn);
    for (int i = 0; i < nn; ++i) par[i] = i;
    const auto find = [&](int a) {
      while (par[a] != a) a = par[a] = par[par[a]];
      return a;
    };
    std::vector<unsigned char> used(nn, 0);
    for (int c = 0; c < nc; ++c)
      for (int q = h_cs[c]; q < h_cs[c + 1]; ++q) {
        if (!h_act[q]) continue;
        const int ne = ro.e_node[c], nf = ro.f_node[h_ot[q]];
        used[ne] = used[nf] = 1;
        const int a = find(ne), b = find(nf);
        if (a != b) par[a] = b;
      }
    std::vector<unsigned char> anchored(nn, 0), needs(nn, 0);
    for (int i = 0; i < nn; ++i) {
      const bool cap = i < ro.n_cap;
      const int role = ro.role(cap, cap ? i : i - ro.n_cap), idx = ro.idx(cap, cap ? i : i - ro.n_cap);
      const bool fr = (role == arslam::kCovE ? cov_e_free(idx) : cov_f_free(idx)) && !cf.is_anchor(role, idx);
      if (fr) needs[find(i)] = 1;
      else if (used[i]) anchored[find(i)] = 1;
    }
    for (int i = 0; i < nn; ++i) deficient = deficient || (needs[i] && !anchored[i]);
  }
  cf.deficient = deficient;
  cf.factored = false;
  arslam_lm_cov_info &info = cf.info;
  info = arslam_lm_cov_info{};
  info.status = ARSLAM_COV_OK;
  info.min_pivot = -1.0;
  info.n_reduced = has_f ? nR : 0;
  info.n_factor_tiles = has_f ? plan.n_tiles : 0;
  if (deficient) return;
  for (auto &e : cov_ev)
    if (!e) HIP_CHECK(hipEventCreate(&e));
  // 1. the linearization at the returned point (jrows; the handle's Jacobi scale stays)
  x = xbest;
  HIP_CHECK(hipEventRecord(cov_ev[0], stream));
  double c0, c1, c2, c3, c4;
  linearize(&c0, &c1, &c2, &c3, &c4);
  HIP_CHECK(hipEventRecord(cov_ev[1], stream));
  // 2. the reduced system with no LM diagonal, eliminated by an orthogonal
  // factorization of each e-block's columns (k_cov_schur: the normal
  // equations' F'F - W'U^-1 W loses cond(U) digits, too many for a
  // covariance), gathered as an LM step's is, then factored.  The gather's
  // diagonal is 0 on the free slots; the camera's l1 / l2 rows, which hold
  // nothing else, get the pivot 1 -- unless they are live: then the border
  // gather writes those rows, and adds this 0
  std::vector<double> dg(n);
  for (long i = 0; i < n; ++i) dg[i] = slot_free[i] ? 0.0 : 1.0;
  dg[1] = dg[2] = cf.live ? 0.0 : 1.0;
  // an anchored call: its scale copy (0 on the anchor and on the direct groups'
  // copies of their captures' slots), the diagonal 1 on the anchor's slots
  std::vector<int> direct;
  if (an) {
    if (cf.anchor_slot >= 0)
      for (int j = 0; j < 6; ++j) {
        h_scale[cf.anchor_slot + j] = 0.0;
        dg[cf.anchor_slot + j] = 1.0;
      }
    if (elim_used == ARSLAM_ELIM_MIXED)
      for (int g = 0; g < nc; ++g)
        if (mx.kind[g] == arslam::kMixDirect) {
          direct.push_back(g);
          std::fill(h_scale.begin() + 3 + 6L * g, h_scale.begin() + 9 + 6L * g, 0.0);
        }
    d_cov_scale.alloc(n);
    d_cov_scale.upload(h_scale.data(), n, stream);
    cf.scale = d_cov_scale.p;
    if (!direct.empty()) {
      d_cov_direct.alloc(direct.size());
      d_cov_direct.upload(direct.data(), direct.size(), stream);
    }
  }
  d_cov_diag.alloc(n);
  HIP_CHECK(hipMemcpyAsync(d_cov_diag.p, dg.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
  d_cov_Q.alloc(std::max(48L * nb, 1L));
  d_cov_Y.alloc(std::max(6L * (nc + 6L * n_blk), 1L));
  d_cov_R.alloc(std::max(36L * nc, 1L));
  arslam::launch_cov_schur(P, cf.scale, d_cov_Q.p, d_cov_Y.p, d_cov_R.p, has_f, stream);
  if (has_f && !direct.empty()) arslam::launch_cov_direct(P, cf.scale, d_cov_direct.p, (int)direct.size(), stream);
  if (cf.live) {
    d_cov_Gl.alloc(12L * std::max(nc, 1));
    arslam::launch_cov_schur_cam(P, CL, cf.scale, d_cov_Q.p, d_cov_Y.p, d_cov_Gl.p, stream);
  }
  if (has_f) {
    const bool dag = opt.factor_executor == 1;
    if (dag) {
      const arslam::LmDiagArgs ld{0, d_scale.p, d_colnorm.p, 0.0, 0.0, d_diag.p, d_yF.p, nR};
      arslam::launch_exec_reset(plan, d_flag.p, stream, &ld);
    } else {
      HIP_CHECK(hipMemsetAsync(d_flag.p, 0, sizeof(int), stream));
    }
    arslam::launch_zero_tiles(plan, Sp, stream);
    arslam::launch_schur_gather(P, d_cov_diag.p, 1.0, Sp, stream);
    if (cf.live) arslam::launch_schur_cam_gather(P, CL, d_cov_diag.p, 1.0, Sp, stream);
    if (!assemble_only) factor_reduced(LONG_MAX, false);   // (every tile was cleared: no first-update store)
    info.n_factor_products = plan.total_upd_tiles + (long)plan.h_gather.size() + plan.T;
  } else {
    HIP_CHECK(hipMemsetAsync(d_flag.p, 0, sizeof(int), stream));
  }
  HIP_CHECK(hipEventRecord(cov_ev[2], stream));
  cf.factored = true;
}

// The calls' one stream sync, behind everything the caller enqueued after
// cov_factor; then the numeric test: no failed pivot, and the smallest squared
// pivot of the real rows (not the padding or the rhs, and l1 / l2 only when
// they are live) at least 1e-14.
void arslam_lm::cov_numeric_test(CovFactor &cf) {
  arslam_lm_cov_info &info = cf.info;
  if (cf.factored) {
    int flag = 0;
    std::vector<double> ld(has_f ? (size_t)plan.T * 4096 : 0);
    HIP_CHECK(hipMemcpyAsync(&flag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    if (has_f) HIP_CHECK(hipMemcpyAsync(ld.data(), plan.ldiag, ld.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (flag < 0) throw Error(ARSLAM_E_DEVICE, executor_fault_message(flag, rank, -1, plan, stream));
    float ms[2] = {0, 0};
    for (int i = 0; i < 2; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], cov_ev[i], cov_ev[i + 1]));
    info.t_linearize_ms = ms[0];
    info.t_factor_ms = ms[1];
    if (flag > 0) {
      cf.deficient = true;
    } else {
      double mp = 1.0;
      bool first = true;
      for (long r = 0; r < (has_f ? nR : 0); ++r) {
        const int sl = lay.row_slot[r];
        if (sl < 0 || (!cf.live && (sl == 1 || sl == 2))) continue;
        if (cf.anchor_slot >= 0 && sl >= cf.anchor_slot && sl < cf.anchor_slot + 6) continue;   // (identity rows)
        const double l = ld[(size_t)(r >> 6) * 4096 + (r & 63) * 65];
        const double p2 = l * l;
        if (first || !(p2 >= mp)) mp = p2;   // (a NaN pivot stays)
        first = false;
      }
      info.min_pivot = mp;
      if (!(mp >= 1e-14)) cf.deficient = true;
    }
  }
  if (cf.deficient) info.status = ARSLAM_COV_RANK_DEFICIENT;
}

// Marginal covariances at the point the last solve returned (arslam_lm.h):
// cov_factor, the selected inverse over the factor's tiles and the two block
// kernels (selinv.hip).  The result is kept on the host in the caller's block
// order.  lens: arslam_lm_covariance_lens -- with l1, l2 live the lens
// instances of the block kernels and the camera's 3x3; held, the same launches
// as without it, var(f) at [0] of the 3x3.
// an: arslam_lm_covariance_anchored -- cov_factor's anchored path, every block
// kernel on the call's scale copy, the anchor's outputs overridden here.
void arslam_lm::covariance(bool lens, const CovAnchor *an) {
  const char *who = an ? "covariance_anchored" : lens ? "covariance_lens" : "covariance";
  cov_check_state(who, lens, an != nullptr);
  if (an) cov_check_anchor(who, *an, cov_roles());
  cov_valid = false;
  cov_anch_valid = false;
  CovFactor cf;
  cov_factor(cf, lens, false, an);
  arslam_lm_cov_info &info = cf.info;
  const int n_cam = cf.live ? 9 : 1;   // the tail of d_cov_out: the camera's 3x3, or var(f)
  std::vector<double> out(36L * nc + 36L * nt + n_cam, -1.0);
  std::vector<int> st_e(std::max(nc, 1), 0);
  if (cf.factored) {
    // 3. the selected inverse on the factor's tiles
    if (has_f) {
      if (!cov_sp_ready) {
        arslam::selinv_plan_build(plan, cov_sp, stream);
        cov_sp_ready = true;
      }
      d_cov_Z.alloc((size_t)plan.n_tiles * 4096);
      arslam::launch_selinv(plan, cov_sp, Sp, nR, d_cov_Z.p, d_flag.p, stream);
      info.n_selinv_products = cov_sp.n_products;
    }
    HIP_CHECK(hipEventRecord(cov_ev[3], stream));
    // 4. the blocks
    d_cov_out.alloc(out.size());
    d_cov_status.alloc(std::max(nc, 1));
    if (cf.live)
      arslam::launch_cov_blocks_lens(P, d_cov_Z.p, cf.scale, d_cov_Y.p, d_cov_R.p, d_cov_Gl.p, d_cov_out.p,
                                     d_cov_status.p, d_cov_out.p + 36L * nc, d_cov_out.p + 36L * nc + 36L * nt, d_flag.p,
                                     stream);
    else
      arslam::launch_cov_blocks(P, has_f ? d_cov_Z.p : nullptr, cf.scale, d_cov_Y.p, d_cov_R.p, d_cov_out.p, d_cov_status.p,
                                d_cov_out.p + 36L * nc, d_cov_out.p + 36L * nc + 36L * nt, d_flag.p, stream);
    HIP_CHECK(hipEventRecord(cov_ev[4], stream));
    HIP_CHECK(hipMemcpyAsync(out.data(), d_cov_out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (nc) HIP_CHECK(hipMemcpyAsync(st_e.data(), d_cov_status.p, nc * sizeof(int), hipMemcpyDeviceToHost, stream));
  }
  cov_numeric_test(cf);
  if (cf.factored) {
    float ms[2] = {0, 0};
    for (int i = 0; i < 2; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], cov_ev[2 + i], cov_ev[3 + i]));
    info.t_selinv_ms = ms[0];
    info.t_blocks_ms = ms[1];
  }
  const bool deficient = cf.deficient;
  if (deficient) std::fill(out.begin(), out.end(), -1.0);
  // statuses in the device problem's order, then the caller's arrays, each
  // block from its role in the device problem (CovRoles; a mixed set's direct
  // groups are nobody's block); the call's anchor is UNAVAILABLE, -1 in its values
  std::vector<int> se(nc), sf(nt);
  for (int c = 0; c < nc; ++c)
    se[c] = !cov_e_free(c) ? ARSLAM_COV_UNAVAILABLE : (deficient || st_e[c] == 2) ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
  for (int t = 0; t < nt; ++t)
    sf[t] = !cov_f_free(t) ? ARSLAM_COV_UNAVAILABLE : deficient ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
  const CovRoles &ro = cf.roles;
  const auto to_caller = [&](bool cap, std::vector<double> &cv, std::vector<int> &sv) {
    const int nblk = cap ? ro.n_cap : ro.n_tag;
    cv.assign(36L * nblk, -1.0);
    sv.assign(nblk, ARSLAM_COV_UNAVAILABLE);
    for (int i = 0; i < nblk; ++i) {
      const int role = ro.role(cap, i), idx = ro.idx(cap, i);
      if (idx < 0 || cf.is_anchor(role, idx)) continue;
      const double *src = out.data() + (role == arslam::kCovE ? 36L * idx : 36L * nc + 36L * idx);
      sv[i] = role == arslam::kCovE ? se[idx] : sf[idx];
      if (sv[i] == ARSLAM_COV_OK) std::copy(src, src + 36, cv.begin() + 36L * i);
    }
  };
  to_caller(true, cov_cap, cov_cap_status);
  to_caller(false, cov_tag, cov_tag_status);
  // the camera: its 3x3 over [f, l1, l2] (held l1, l2: their rows and columns 0), and var(f)
  const double *tail = out.data() + 36L * (nc + nt);
  const bool cam_free = has_f && P.cam_row >= 0;
  cov_cam_status = !cam_free ? ARSLAM_COV_UNAVAILABLE : deficient ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
  if (cov_cam_status != ARSLAM_COV_OK) {
    std::fill(cov_cam, cov_cam + 9, -1.0);
  } else if (cf.live) {
    std::copy(tail, tail + 9, cov_cam);
  } else {
    std::fill(cov_cam, cov_cam + 9, 0.0);
    cov_cam[0] = tail[0];
  }
  cov_var_f = cf.live ? cov_cam[0] : tail[0];
  cov_from_lens = lens;
  cov_info = info;
  cov_valid = an == nullptr;
  cov_anch_valid = an != nullptr;
  if (an) cov_anch = *an;
}

// Cross-covariance blocks of the same matrix (arslam_lm.h): cov_factor, then
// whole columns of Z = S^-1 by the multi-right-hand-side tile solve
// (cov_pairs.hip) on the factor itself -- this call never runs the selected
// inverse, whose first kernel overwrites the off-diagonal factor tiles in
// place, and it refactors every time, so an earlier covariance() leaves it
// nothing to trip over.  Each unordered pair is computed once, with the block
// of the smaller key (the focal, then the reduced side's blocks, then the
// eliminated side's, by index) as the solved side; the other order is its
// transpose.  The distinct solved blocks go through the solve in batches of at
// most kCovBatchPanels panels and kCovBatchBytes.  A right-hand side is
// non-zero only in the tile rows of its block, so the forward pass touches
// their ancestors in the elimination tree and nothing else, and the backward
// pass computes only the tile rows some pair of the panel reads (and their
// ancestors): per-panel byte masks, built here.
// lens: arslam_lm_covariance_pairs_lens -- the camera's block is [f, l1, l2];
// with l1, l2 live its right-hand side is three unit columns and the lens
// instances of the two small kernels run (cov_lens.hip).
void arslam_lm::covariance_pairs(const arslam_lm_cov_pair *pairs, int n_pairs, double *cov, int *status,
                                 arslam_lm_cov_info *info_out, bool lens, const CovAnchor *an) {
  const char *who = an ? "covariance_pairs_anchored" : lens ? "covariance_pairs_lens" : "covariance_pairs";
  cov_check_state(who, lens, an != nullptr);
  const CovRoles ro = cov_roles();
  if (an) cov_check_anchor(who, *an, ro);
  const int n_caller_cap = ro.n_cap, n_caller_tag = ro.n_tag;
  // the caller's block in the device problem: {role, idx} (CovRoles: per block, under any e-block set)
  struct Blk {
    int role, idx;
    long key() const { return role == arslam::kCovFocal ? 0L : role == arslam::kCovF ? 1L + idx : (1L << 40) + idx; }
  };
  const auto device_block = [&](int kind, int index) -> Blk {
    fail_if(kind != ARSLAM_BLOCK_CAMERA && kind != ARSLAM_BLOCK_CAPTURE && kind != ARSLAM_BLOCK_TAG,
            ARSLAM_E_INVALID_ARG, "covariance_pairs: kind must be ARSLAM_BLOCK_CAMERA, _CAPTURE or _TAG");
    if (kind == ARSLAM_BLOCK_CAMERA) {
      fail_if(index != 0, ARSLAM_E_INVALID_ARG, "covariance_pairs: the camera's index is 0");
      return Blk{arslam::kCovFocal, 0};
    }
    const bool cap = kind == ARSLAM_BLOCK_CAPTURE;
    fail_if(index < 0 || index >= (cap ? n_caller_cap : n_caller_tag), ARSLAM_E_INVALID_ARG,
            "covariance_pairs: block index out of range");
    return Blk{ro.role(cap, index), ro.idx(cap, index)};
  };
  std::vector<Blk> blk(2L * n_pairs);
  for (int i = 0; i < n_pairs; ++i) {
    blk[2L * i] = device_block(pairs[i].kind_a, pairs[i].index_a);
    blk[2L * i + 1] = device_block(pairs[i].kind_b, pairs[i].index_b);
  }
  CovFactor cf;
  cov_factor(cf, lens, false, an);
  const bool live = cf.live;
  const auto available = [&](const Blk &b) {
    if (b.role == arslam::kCovFocal) return has_f && P.cam_row >= 0;
    if (cf.is_anchor(b.role, b.idx)) return false;   // (held fixed for this call)
    if (b.role == arslam::kCovF)
      return has_f && cov_f_free(b.idx) && (size_t)b.idx < lay.tag_row.size() && lay.tag_row[b.idx] >= 0;
    return cov_e_free(b.idx) && cf.cap_start[b.idx + 1] > cf.cap_start[b.idx];
  };
  // the distinct unordered pairs of available blocks, keyed (solved side, other side): in batch order
  std::map<std::pair<long, long>, int> task_of;
  std::vector<unsigned char> avail(n_pairs, 0);
  for (int i = 0; i < n_pairs; ++i) {
    avail[i] = available(blk[2L * i]) && available(blk[2L * i + 1]);
    if (!avail[i]) continue;
    const long ka = blk[2L * i].key(), kb = blk[2L * i + 1].key();
    task_of.emplace(std::make_pair(std::min(ka, kb), std::max(ka, kb)), 0);
  }
  const auto block_of = [&](long key) -> Blk {
    return key == 0 ? Blk{arslam::kCovFocal, 0}
                    : key < (1L << 40) ? Blk{arslam::kCovF, (int)(key - 1)} : Blk{arslam::kCovE, (int)(key - (1L << 40))};
  };
  std::vector<arslam::CovPairTask> tasks;
  std::vector<int2> rhs;
  std::vector<int> task_rhs;   // the solved block's position in rhs
  {
    long last = -1;
    for (auto &kv : task_of) {
      const Blk b = block_of(kv.first.first), a = block_of(kv.first.second);
      if (rhs.empty() || kv.first.first != last) rhs.push_back(make_int2(b.role, b.idx));
      last = kv.first.first;
      kv.second = (int)tasks.size();
      task_rhs.push_back((int)rhs.size() - 1);
      tasks.push_back(arslam::CovPairTask{a.role, a.idx, b.role, b.idx, 0, (int)tasks.size()});
    }
  }
  const int n_tasks = (int)tasks.size(), n_rhs = (int)rhs.size();
  // panels per batch: what fits kCovBatchBytes, kCovBatchPanels at most (a panel is T x 32 KB)
  const size_t panel = (size_t)std::max(plan.T, 1) * 4096;
  const int batch_panels = (int)std::min<size_t>(kCovBatchPanels, std::max<size_t>(1, kCovBatchBytes / (panel * sizeof(double))));
  const int per_batch = batch_panels * arslam::kCovPanelBlocks;
  for (int t = 0; t < n_tasks; ++t) tasks[t].slot = task_rhs[t] % per_batch;
  std::vector<double> out(36L * std::max(n_tasks, 1), -1.0);
  std::vector<int> st(std::max(n_tasks, 1), 2);
  arslam_lm_cov_info &info = cf.info;
  const int n_batches = (n_rhs + per_batch - 1) / per_batch;
  const bool run = cf.factored && n_tasks > 0;
  if (run) {
    const int T = plan.T;
    const int all_panels = (n_rhs + arslam::kCovPanelBlocks - 1) / arslam::kCovPanelBlocks;   // (a batch holds whole panels)
    // per panel, the tile rows its right-hand sides touch (active) and those its pairs read (needed)
    std::vector<unsigned char> mask(has_f ? 2 * (size_t)all_panels * T : 0, 0);
    unsigned char *active = mask.data(), *needed = mask.data() + (size_t)all_panels * T;
    if (has_f) {
      if (!cov_tp_ready) {
        arslam::tile_solve_plan_build(plan, cov_tp, stream);
        cov_tp_ready = true;
      }
      // the e-blocks' local f-blocks (their reduced rows are where an e-block's columns and rows live)
      std::vector<int> h_bs(nc + 1, 0), h_bt;
      bool any_e = false;
      for (const auto &t : tasks) any_e = any_e || t.role_a == arslam::kCovE || t.role_b == arslam::kCovE;
      if (any_e) {
        HIP_CHECK(hipMemcpyAsync(h_bs.data(), u_cap_blk_start, (nc + 1) * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        h_bt.resize(std::max(h_bs[nc], 1));
        if (h_bs[nc]) HIP_CHECK(hipMemcpyAsync(h_bt.data(), u_blk_tag, h_bs[nc] * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
      }
      const auto f_row = [&](int t) -> long { return (size_t)t < lay.tag_row.size() ? lay.tag_row[t] : -1; };
      const auto mark = [&](unsigned char *m, int role, int idx) {
        const auto rows6 = [&](long r) {
          if (r < 0) return;
          arslam::tile_solve_mark(cov_tp, m, r);
          arslam::tile_solve_mark(cov_tp, m, r + 5);
        };
        // (the camera's three live rows may straddle a tile boundary)
        const auto cam_rows = [&] {
          if (P.cam_row < 0) return;
          arslam::tile_solve_mark(cov_tp, m, P.cam_row);
          if (live) arslam::tile_solve_mark(cov_tp, m, P.cam_row + 2);
        };
        if (role == arslam::kCovFocal) {
          cam_rows();
        } else if (role == arslam::kCovF) {
          rows6(f_row(idx));
        } else {
          cam_rows();
          for (int u = h_bs[idx]; u < h_bs[idx + 1]; ++u) rows6(f_row(h_bt[u]));
        }
      };
      for (int r = 0; r < n_rhs; ++r) mark(active + (size_t)(r / arslam::kCovPanelBlocks) * T, rhs[r].x, rhs[r].y);
      for (int t = 0; t < n_tasks; ++t)
        mark(needed + (size_t)(task_rhs[t] / arslam::kCovPanelBlocks) * T, tasks[t].role_a, tasks[t].idx_a);
      d_pair_mask.alloc(mask.size());
      d_pair_mask.upload(mask.data(), mask.size(), stream);
      d_pair_B.alloc(panel * std::min(batch_panels, all_panels));
      while ((int)pair_ev.size() < 2 * n_batches) {
        hipEvent_t e = nullptr;
        HIP_CHECK(hipEventCreate(&e));
        pair_ev.push_back(e);
      }
    }
    d_pair_rhs.alloc(n_rhs);
    d_pair_tasks.alloc(n_tasks);
    d_pair_out.alloc(36L * n_tasks);
    d_pair_status.alloc(n_tasks);
    d_pair_rhs.upload(rhs.data(), n_rhs, stream);
    d_pair_tasks.upload(tasks.data(), n_tasks, stream);
    int t0 = 0;
    for (int bt = 0; bt < n_batches; ++bt) {
      const int r0 = bt * per_batch, nr = std::min(per_batch, n_rhs - r0);
      const int np = (nr + arslam::kCovPanelBlocks - 1) / arslam::kCovPanelBlocks;
      int t1 = t0;
      while (t1 < n_tasks && task_rhs[t1] < r0 + nr) ++t1;
      if (has_f) {
        const size_t m0 = (size_t)bt * batch_panels * T;   // this batch's first panel in the masks
        HIP_CHECK(hipMemsetAsync(d_pair_B.p, 0, panel * np * sizeof(double), stream));
        if (live) arslam::launch_cov_pair_rhs_lens(P, d_cov_Y.p, d_cov_R.p, d_cov_Gl.p, d_pair_rhs.p + r0, nr, d_pair_B.p, stream);
        else arslam::launch_cov_pair_rhs(P, d_cov_Y.p, d_cov_R.p, d_pair_rhs.p + r0, nr, d_pair_B.p, stream);
        HIP_CHECK(hipEventRecord(pair_ev[2 * bt], stream));
        arslam::launch_tile_solve(plan, cov_tp, Sp, nR, d_pair_B.p, np, d_pair_mask.p + m0,
                                  d_pair_mask.p + (size_t)all_panels * T + m0, d_flag.p, stream);
        HIP_CHECK(hipEventRecord(pair_ev[2 * bt + 1], stream));
        for (int p = 0; p < np; ++p)
          info.n_selinv_products += arslam::tile_solve_products(plan, cov_tp, active + m0 + (size_t)p * T, needed + m0 + (size_t)p * T);
      }
      if (live)
        arslam::launch_cov_pair_blocks_lens(P, d_pair_B.p, cf.scale, d_cov_Y.p, d_cov_R.p, d_cov_Gl.p, d_pair_tasks.p + t0,
                                            t1 - t0, d_pair_out.p, d_pair_status.p, d_flag.p, stream);
      else
        arslam::launch_cov_pair_blocks(P, has_f ? d_pair_B.p : nullptr, cf.scale, d_cov_Y.p, d_cov_R.p, d_pair_tasks.p + t0,
                                       t1 - t0, d_pair_out.p, d_pair_status.p, d_flag.p, stream);
      t0 = t1;
    }
    HIP_CHECK(hipEventRecord(cov_ev[3], stream));
    HIP_CHECK(hipMemcpyAsync(out.data(), d_pair_out.p, 36L * n_tasks * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(st.data(), d_pair_status.p, n_tasks * sizeof(int), hipMemcpyDeviceToHost, stream));
  }
  cov_numeric_test(cf);
  if (run) {
    float all = 0.f, solve = 0.f;
    HIP_CHECK(hipEventElapsedTime(&all, cov_ev[2], cov_ev[3]));
    for (int bt = 0; has_f && bt < n_batches; ++bt) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, pair_ev[2 * bt], pair_ev[2 * bt + 1]));
      solve += ms;
    }
    info.t_selinv_ms = solve;
    info.t_blocks_ms = std::max(0.f, all - solve);
  }
  // the caller's pairs: its (a, b) as computed or transposed; the focal's 6 values
  // first -- the lens form: the camera's rows (as a) or columns (as b), 3 when live
  const int n_camv = live ? 3 : 1;
  for (int i = 0; i < n_pairs; ++i) {
    double *c = cov + 36L * i;
    int s = ARSLAM_COV_UNAVAILABLE;
    if (avail[i]) {
      const Blk &ba = blk[2L * i], &bb = blk[2L * i + 1];
      const long ka = ba.key(), kb = bb.key();
      const int t = task_of.at(std::make_pair(std::min(ka, kb), std::max(ka, kb)));
      s = (cf.deficient || st[t] != 0) ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
      if (s == ARSLAM_COV_OK) {
        const double *o = out.data() + 36L * t;   // rows: the larger key's block; columns: the smaller's
        const bool as_is = ka >= kb;
        double m[36];
        for (int r = 0; r < 6; ++r)
          for (int q = 0; q < 6; ++q) m[6 * r + q] = as_is ? o[6 * r + q] : o[6 * q + r];
        const bool fa = ba.role == arslam::kCovFocal, fb = bb.role == arslam::kCovFocal;
        std::fill(c, c + 36, 0.0);
        if (lens) {
          const int ra = fa ? n_camv : 6, cb = fb ? n_camv : 6;
          for (int r = 0; r < ra; ++r) std::copy(m + 6 * r, m + 6 * r + cb, c + 6 * r);
        } else if (fa) std::copy(m, m + (fb ? 1 : 6), c);          // row 0: cov(f, b)
        else if (fb) for (int r = 0; r < 6; ++r) c[r] = m[6 * r];   // column 0: cov(a, f)
        else std::copy(m, m + 36, c);
      }
    }
    if (s != ARSLAM_COV_OK) std::fill(c, c + 36, -1.0);
    if (status) status[i] = s;
  }
  if (info_out) *info_out = info;
}
