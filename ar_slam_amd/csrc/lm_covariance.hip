// lm_covariance.hip -- arslam_lm_covariance on the LM handle (lm_handle.h).
#include "lm_handle.h"

// Marginal covariances at the point the last solve returned (arslam_lm.h): the
// structural gauge check on the host, then one linearization, the reduced
// system without the LM diagonal (its own elimination kernel, the LM step's
// gather) and its factorization as in an LM step, the selected inverse over
// the factor's tiles and the two block kernels (selinv.hip).  Everything it writes on the device is scratch the next
// solve rebuilds from the loaded state; the result is kept on the host in the
// caller's block order.
void arslam_lm::covariance() {
  fail_if(!loaded || solve_state == 0, ARSLAM_E_STATE, "covariance: no completed solve of the loaded problem");
  fail_if(solve_state == 2, ARSLAM_E_STATE, "covariance: the last solve ended with rule EVAL_FAILED");
  fail_if(multi(), ARSLAM_E_UNSUPPORTED, "covariance: single-rank only");
  fail_if(elim_used == ARSLAM_ELIM_MIXED, ARSLAM_E_UNSUPPORTED,
          "covariance: the mixed e-block set is not supported (ARSLAM_ELIM_CAPTURES or _TAGS)");
  cov_valid = false;
  ensure_stream();
  // the device problem's structure (its host copy is not kept after a load)
  std::vector<int> h_cs(nc + 1, 0), h_ot(std::max(nb, 1));
  std::vector<unsigned char> h_act(std::max(nb, 1));
  int n_blk = 0;
  HIP_CHECK(hipMemcpyAsync(h_cs.data(), u_cap_start, (nc + 1) * sizeof(int), hipMemcpyDeviceToHost, stream));
  if (nb) HIP_CHECK(hipMemcpyAsync(h_ot.data(), u_obs_tag, nb * sizeof(int), hipMemcpyDeviceToHost, stream));
  if (nb) HIP_CHECK(hipMemcpyAsync(h_act.data(), u_obs_active, nb, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(&n_blk, u_cap_blk_start + nc, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  // Gauge: every connected component of the e-block / f-block graph over the
  // active observations that holds a free block must hold a constant one
  const auto e_free = [&](int c) { return slot_free[3 + 6L * c] != 0; };
  const auto f_free = [&](int t) { return slot_free[3 + 6L * nc + 6L * t] != 0; };
  bool deficient = false;
  {
    std::vector<int> par(nc + nt);
    for (int i = 0; i < nc + nt; ++i) par[i] = i;
    const auto find = [&](int a) {
      while (par[a] != a) a = par[a] = par[par[a]];
      return a;
    };
    std::vector<unsigned char> used(nc + nt, 0);
    for (int c = 0; c < nc; ++c)
      for (int q = h_cs[c]; q < h_cs[c + 1]; ++q) {
        if (!h_act[q]) continue;
        used[c] = used[nc + h_ot[q]] = 1;
        const int a = find(c), b = find(nc + h_ot[q]);
        if (a != b) par[a] = b;
      }
    std::vector<unsigned char> anchored(nc + nt, 0), needs(nc + nt, 0);
    for (int i = 0; i < nc + nt; ++i) {
      const bool fr = i < nc ? e_free(i) : f_free(i - nc);
      if (fr) needs[find(i)] = 1;
      else if (used[i]) anchored[find(i)] = 1;
    }
    for (int i = 0; i < nc + nt; ++i) deficient = deficient || (needs[i] && !anchored[i]);
  }
  std::vector<double> out(36L * nc + 36L * nt + 1, -1.0);
  std::vector<int> st_e(std::max(nc, 1), 0);
  arslam_lm_cov_info info{};
  info.status = ARSLAM_COV_OK;
  info.min_pivot = -1.0;
  info.n_reduced = has_f ? nR : 0;
  info.n_factor_tiles = has_f ? plan.n_tiles : 0;
  if (!deficient) {
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
    // nothing else, get the pivot 1
    std::vector<double> dg(n);
    for (long i = 0; i < n; ++i) dg[i] = slot_free[i] ? 0.0 : 1.0;
    dg[1] = dg[2] = 1.0;
    d_cov_diag.alloc(n);
    HIP_CHECK(hipMemcpyAsync(d_cov_diag.p, dg.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
    d_cov_Q.alloc(std::max(48L * nb, 1L));
    d_cov_Y.alloc(std::max(6L * (nc + 6L * n_blk), 1L));
    d_cov_R.alloc(std::max(36L * nc, 1L));
    arslam::launch_cov_schur(P, d_scale.p, d_cov_Q.p, d_cov_Y.p, d_cov_R.p, has_f, stream);
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
      factor_reduced(LONG_MAX, false);   // (every tile was cleared: no first-update store)
    } else {
      HIP_CHECK(hipMemsetAsync(d_flag.p, 0, sizeof(int), stream));
    }
    HIP_CHECK(hipEventRecord(cov_ev[2], stream));
    // 3. the selected inverse on the factor's tiles
    if (has_f) {
      if (!cov_sp_ready) {
        arslam::selinv_plan_build(plan, cov_sp, stream);
        cov_sp_ready = true;
      }
      d_cov_Z.alloc((size_t)plan.n_tiles * 4096);
      arslam::launch_selinv(plan, cov_sp, Sp, nR, d_cov_Z.p, d_flag.p, stream);
      info.n_selinv_products = cov_sp.n_products;
      info.n_factor_products = plan.total_upd_tiles + (long)plan.h_gather.size() + plan.T;
    }
    HIP_CHECK(hipEventRecord(cov_ev[3], stream));
    // 4. the blocks
    d_cov_out.alloc(out.size());
    d_cov_status.alloc(std::max(nc, 1));
    arslam::launch_cov_blocks(P, has_f ? d_cov_Z.p : nullptr, d_scale.p, d_cov_Y.p, d_cov_R.p, d_cov_out.p, d_cov_status.p,
                              d_cov_out.p + 36L * nc, d_cov_out.p + 36L * nc + 36L * nt, d_flag.p, stream);
    HIP_CHECK(hipEventRecord(cov_ev[4], stream));
    int flag = 0;
    std::vector<double> ld(has_f ? (size_t)plan.T * 4096 : 0);
    HIP_CHECK(hipMemcpyAsync(out.data(), d_cov_out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (nc) HIP_CHECK(hipMemcpyAsync(st_e.data(), d_cov_status.p, nc * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(&flag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    if (has_f) HIP_CHECK(hipMemcpyAsync(ld.data(), plan.ldiag, ld.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (flag < 0) throw Error(ARSLAM_E_DEVICE, executor_fault_message(flag, rank, -1, plan, stream));
    float ms[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], cov_ev[i], cov_ev[i + 1]));
    info.t_linearize_ms = ms[0];
    info.t_factor_ms = ms[1];
    info.t_selinv_ms = ms[2];
    info.t_blocks_ms = ms[3];
    // the numeric test: no failed pivot, and the smallest squared pivot of the
    // real rows (not l1 / l2, the padding or the rhs) at least 1e-14
    if (flag > 0) {
      deficient = true;
    } else {
      double mp = 1.0;
      bool first = true;
      for (long r = 0; r < (has_f ? nR : 0); ++r) {
        const int sl = lay.row_slot[r];
        if (sl < 0 || sl == 1 || sl == 2) continue;
        const double l = ld[(size_t)(r >> 6) * 4096 + (r & 63) * 65];
        const double p2 = l * l;
        if (first || !(p2 >= mp)) mp = p2;   // (a NaN pivot stays)
        first = false;
      }
      info.min_pivot = mp;
      if (!(mp >= 1e-14)) deficient = true;
    }
  }
  if (deficient) {
    info.status = ARSLAM_COV_RANK_DEFICIENT;
    std::fill(out.begin(), out.end(), -1.0);
  }
  // statuses in the device problem's order, then the caller's arrays (tag
  // elimination: the e-blocks are the caller's tags)
  std::vector<int> se(nc), sf(nt);
  for (int c = 0; c < nc; ++c)
    se[c] = !e_free(c) ? ARSLAM_COV_UNAVAILABLE : (deficient || st_e[c] == 2) ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
  for (int t = 0; t < nt; ++t)
    sf[t] = !f_free(t) ? ARSLAM_COV_UNAVAILABLE : deficient ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
  const bool swapped = elim_used == ARSLAM_ELIM_TAGS;
  std::vector<double> ce(out.begin(), out.begin() + 36L * nc), cf(out.begin() + 36L * nc, out.begin() + 36L * (nc + nt));
  cov_cap = swapped ? cf : ce;
  cov_tag = swapped ? ce : cf;
  cov_cap_status = swapped ? sf : se;
  cov_tag_status = swapped ? se : sf;
  cov_var_f = out.back();
  cov_info = info;
  cov_valid = true;
}
