// lm_covariance.hip -- the covariances of the LM handle (lm_handle.h): covariance() and covariance_pairs()
// for every form of the call (CovForm: plain, _lens, _anchored -- a pose block held fixed for the call; any
// e-block set), the one map between the caller's blocks and the device problem's (BlockMap), and what the
// two share (cov_factor, cov_numeric_test), each in stages.  The entry points are lm_cov_capi.hip's.
#include "lm_handle.h"

#include <map>

void arslam_lm::cov_check_state(const std::string &w, const CovForm &form) const {
  fail_if(!form.lens && est_active(), ARSLAM_E_UNSUPPORTED,
          w + ": not supported while estimate_distortion is on (its camera output is one scalar: use the _lens form)");
  fail_if(!loaded || solve_state == 0, ARSLAM_E_STATE, w + ": no completed solve of the loaded problem");
  fail_if(solve_state == 2, ARSLAM_E_STATE, w + ": the last solve ended with rule EVAL_FAILED");
  fail_if(multi(), ARSLAM_E_UNSUPPORTED, w + ": single-rank only");
  fail_if(!form.anchored && elim_used == ARSLAM_ELIM_MIXED, ARSLAM_E_UNSUPPORTED,
          w + ": the mixed e-block set is not supported (ARSLAM_ELIM_CAPTURES or _TAGS, or the _anchored form)");
}

arslam_lm::BlockMap arslam_lm::block_map() const {
  BlockMap bm;
  const auto size = [&](int n_cap, int n_tag) {
    bm.n_cap = n_cap;
    bm.n_tag = n_tag;
    bm.cap_role.assign(n_cap, arslam::kCovF);
    bm.cap_idx.assign(n_cap, -1);
    bm.tag_role.assign(n_tag, arslam::kCovF);
    bm.tag_idx.assign(n_tag, -1);
    bm.e_node.assign(nc, -1);
    bm.f_node.assign(nt, -1);
  };
  const auto put = [&](bool cap, int i, int role, int idx) {
    (cap ? bm.cap_role : bm.tag_role)[i] = role;
    (cap ? bm.cap_idx : bm.tag_idx)[i] = idx;
    (role == arslam::kCovE ? bm.e_node : bm.f_node)[idx] = cap ? i : bm.n_cap + i;
  };
  if (elim_used == ARSLAM_ELIM_MIXED) {
    size(mx.src_n_cap, mx.src_n_tag);
    for (int f = 0; f < nt; ++f) put(mx.f_is_cap[f] != 0, mx.f_src[f], arslam::kCovF, f);
    for (int g = 0; g < nc; ++g) {
      if (mx.kind[g] == arslam::kMixDirect) bm.e_node[g] = mx.group_src[g];   // (its capture: an f-block)
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
  return bm;
}

void arslam_lm::cov_check_anchor(const std::string &w, const CovForm &form, const BlockMap &bm) const {
  if (!form.anchored) return;
  const CovAnchor &an = form.anchor;
  fail_if(an.kind != ARSLAM_BLOCK_NONE && an.kind != ARSLAM_BLOCK_CAPTURE && an.kind != ARSLAM_BLOCK_TAG,
          ARSLAM_E_INVALID_ARG, w + ": the anchor's kind must be ARSLAM_BLOCK_CAPTURE, _TAG or _NONE");
  if (an.none()) return;
  const int nblk = an.kind == ARSLAM_BLOCK_CAPTURE ? bm.n_cap : bm.n_tag;
  fail_if(an.index < 0 || an.index >= nblk, ARSLAM_E_INVALID_ARG, w + ": the anchor's index is out of range");
}

// cov_factor's stage 1: the device problem's structure (its host copy is not
// kept after a load) and, for an anchored form, the Jacobi scale to copy
struct arslam_lm::CovStructure {
  std::vector<int> obs_tag;
  std::vector<unsigned char> obs_active;
  int n_blk = 0;               // the e-blocks' local f-blocks, all told
  std::vector<double> scale;   // (an anchored form)
};

void arslam_lm::cov_read_structure(CovFactor &cf, const CovForm &form, CovStructure &st) {
  st.scale.resize(form.anchored ? n : 0);
  if (form.anchored) HIP_CHECK(hipMemcpyAsync(st.scale.data(), d_scale.p, n * sizeof(double), hipMemcpyDeviceToHost, stream));
  cf.cap_start.assign(nc + 1, 0);
  st.obs_tag.resize(std::max(nb, 1));
  st.obs_active.resize(std::max(nb, 1));
  HIP_CHECK(hipMemcpyAsync(cf.cap_start.data(), u_cap_start, (nc + 1) * sizeof(int), hipMemcpyDeviceToHost, stream));
  if (nb) HIP_CHECK(hipMemcpyAsync(st.obs_tag.data(), u_obs_tag, nb * sizeof(int), hipMemcpyDeviceToHost, stream));
  if (nb) HIP_CHECK(hipMemcpyAsync(st.obs_active.data(), u_obs_active, nb, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(&st.n_blk, u_cap_blk_start + nc, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
}

namespace {
// cov_factor's stage 2, on the host alone.  Gauge: every connected component
// of the caller's capture / tag graph over the active observations that holds a
// free block must hold a constant one (is_free(role, idx): the call's anchor
// counts as constant).  An observation joins the caller's blocks of its group
// and its f-block (BlockMap: a direct group's is its capture, no block of its
// own), so the outcome does not depend on the e-block set.
template <class Free>
bool gauge_deficient(const arslam_lm::BlockMap &bm, const std::vector<int> &cap_start, const std::vector<int> &obs_tag,
                     const std::vector<unsigned char> &obs_active, const Free &is_free) {
  const int nn = bm.n_cap + bm.n_tag;
  std::vector<int> par(nn);
  for (int i = 0; i < nn; ++i) par[i] = i;
  const auto find = [&](int a) {
    while (par[a] != a) a = par[a] = par[par[a]];
    return a;
  };
  std::vector<unsigned char> used(nn, 0);
  for (size_t c = 0; c + 1 < cap_start.size(); ++c)
    for (int q = cap_start[c]; q < cap_start[c + 1]; ++q) {
      if (!obs_active[q]) continue;
      const int ne = bm.e_node[c], nf = bm.f_node[obs_tag[q]];
      used[ne] = used[nf] = 1;
      const int a = find(ne), b = find(nf);
      if (a != b) par[a] = b;
    }
  std::vector<unsigned char> anchored(nn, 0), needs(nn, 0);
  for (int i = 0; i < nn; ++i) {
    const bool cap = i < bm.n_cap;
    if (is_free(bm.role(cap, cap ? i : i - bm.n_cap), bm.idx(cap, cap ? i : i - bm.n_cap))) needs[find(i)] = 1;
    else if (used[i]) anchored[find(i)] = 1;
  }
  bool deficient = false;
  for (int i = 0; i < nn; ++i) deficient = deficient || (needs[i] && !anchored[i]);
  return deficient;
}
}  // namespace

// The structure read back and the gauge check, then (cov_enqueue) one
// linearization at the point the last solve returned, the reduced system
// without the LM diagonal (its own elimination kernel, the LM step's gather)
// and its factorization as in an LM step.  Everything it writes on the device
// is scratch the next solve rebuilds from the loaded state.  A lens form on a
// problem whose l1, l2 are live: they are rows of H like f -- k_cov_schur_cam's
// border and the LM step's border gather put them into the reduced system
// (cov_lens.hip).  assemble_only (arslam_lm_debug_cov_camera_rows): stop before
// the factorization.
//
// An anchored form: the call's anchor is held fixed without an elimination of
// its own.  Every covariance kernel reads a copy of the Jacobi scale with 0 on
// the anchor's six slots: an anchored e-block takes the constant e-block's path
// (Q = 0, G = 0), an anchored f-block's columns vanish and the gather's
// diagonal 1 makes its rows decoupled identity rows; the callers override the
// anchor's outputs.  Under a mixed e-block set the copy is 0 on the direct
// groups' slots too -- k_cov_schur then leaves them no Q, G or R -- and
// k_cov_direct stores their local systems (cov_direct.hip).
void arslam_lm::cov_factor(CovFactor &cf, const CovForm &form, const BlockMap &bm, bool assemble_only) {
  ensure_stream();
  cf.live = form.lens && est_loaded;
  cf.scale = d_scale.p;
  if (form.anchored && !form.anchor.none()) {
    const bool cap = form.anchor.kind == ARSLAM_BLOCK_CAPTURE;
    cf.anchor_role = bm.role(cap, form.anchor.index);
    cf.anchor_idx = bm.idx(cap, form.anchor.index);
    cf.anchor_slot = cf.anchor_role == arslam::kCovE ? 3 + 6L * cf.anchor_idx : 3 + 6L * nc + 6L * cf.anchor_idx;
  }
  CovStructure st;
  cov_read_structure(cf, form, st);
  cf.deficient = gauge_deficient(bm, cf.cap_start, st.obs_tag, st.obs_active, [&](int role, int idx) {
    return (role == arslam::kCovE ? cov_e_free(idx) : cov_f_free(idx)) && !cf.is_anchor(role, idx);
  });
  cf.factored = false;
  cf.info = arslam_lm_cov_info{};
  cf.info.status = ARSLAM_COV_OK;
  cf.info.min_pivot = -1.0;
  cf.info.n_reduced = has_f ? nR : 0;
  cf.info.n_factor_tiles = has_f ? plan.n_tiles : 0;
  if (!cf.deficient) cov_enqueue(cf, form, st, assemble_only);
}

void arslam_lm::cov_enqueue(CovFactor &cf, const CovForm &form, CovStructure &st, bool assemble_only) {
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
  if (form.anchored) {
    if (cf.anchor_slot >= 0)
      for (int j = 0; j < 6; ++j) {
        st.scale[cf.anchor_slot + j] = 0.0;
        dg[cf.anchor_slot + j] = 1.0;
      }
    if (elim_used == ARSLAM_ELIM_MIXED)
      for (int g = 0; g < nc; ++g)
        if (mx.kind[g] == arslam::kMixDirect) {
          direct.push_back(g);
          std::fill(st.scale.begin() + 3 + 6L * g, st.scale.begin() + 9 + 6L * g, 0.0);
        }
    d_cov_scale.alloc(n);
    d_cov_scale.upload(st.scale.data(), n, stream);
    cf.scale = d_cov_scale.p;
    if (!direct.empty()) {
      d_cov_direct.alloc(direct.size());
      d_cov_direct.upload(direct.data(), direct.size(), stream);
    }
  }
  d_cov_diag.alloc(n);
  HIP_CHECK(hipMemcpyAsync(d_cov_diag.p, dg.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
  d_cov_Q.alloc(std::max(48L * nb, 1L));
  d_cov_Y.alloc(std::max(6L * (nc + 6L * st.n_blk), 1L));
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
    cf.info.n_factor_products = plan.total_upd_tiles + (long)plan.h_gather.size() + plan.T;
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
// order, with its form.  A lens form: with l1, l2 live the lens instances of the
// block kernels and the camera's 3x3; held, the same launches as without it,
// var(f) at [0] of the 3x3.  An anchored form: cov_factor's anchored path, every
// block kernel on the call's scale copy, the anchor's outputs overridden here.
void arslam_lm::covariance(const CovForm &form) {
  const std::string who = form.name("covariance");
  cov_check_state(who, form);
  const BlockMap bm = block_map();
  cov_check_anchor(who, form, bm);
  cov_kept = false;
  CovFactor cf;
  cov_factor(cf, form, bm);
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
  // block from its role in the device problem (BlockMap; a mixed set's direct
  // groups are nobody's block); the call's anchor is UNAVAILABLE, -1 in its values
  std::vector<int> se(nc), sf(nt);
  for (int c = 0; c < nc; ++c)
    se[c] = !cov_e_free(c) ? ARSLAM_COV_UNAVAILABLE : (deficient || st_e[c] == 2) ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
  for (int t = 0; t < nt; ++t)
    sf[t] = !cov_f_free(t) ? ARSLAM_COV_UNAVAILABLE : deficient ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
  const auto to_caller = [&](bool cap, std::vector<double> &cv, std::vector<int> &sv) {
    const int nblk = cap ? bm.n_cap : bm.n_tag;
    cv.assign(36L * nblk, -1.0);
    sv.assign(nblk, ARSLAM_COV_UNAVAILABLE);
    for (int i = 0; i < nblk; ++i) {
      const int role = bm.role(cap, i), idx = bm.idx(cap, i);
      if (idx < 0 || cf.is_anchor(role, idx)) continue;
      const double *src = out.data() + 36L * bm.device_block(cap, i, nc);
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
  cov_info = info;
  cov_form = form;
  cov_kept = true;
}

// covariance_pairs' plan, stage by stage.  A block of the device problem is
// {role, idx}; its key orders the focal first, then the reduced side's blocks,
// then the eliminated side's, by index.
struct arslam_lm::CovPairPlan {
  struct Blk {
    int role, idx;
    long key() const { return role == arslam::kCovFocal ? 0L : role == arslam::kCovF ? 1L + idx : (1L << 40) + idx; }
    static Blk of_key(long key) {
      return key == 0 ? Blk{arslam::kCovFocal, 0}
                      : key < (1L << 40) ? Blk{arslam::kCovF, (int)(key - 1)} : Blk{arslam::kCovE, (int)(key - (1L << 40))};
    }
  };
  // 1. the caller's pairs: their blocks (a, b per pair) and whether both are available
  std::vector<Blk> blk;
  std::vector<unsigned char> avail;
  // 2. the distinct unordered pairs of available blocks, keyed (solved side,
  // other side), in batch order; the distinct solved blocks; each task's
  // solved block in rhs.  A batch solves per_batch blocks in batch_panels panels.
  std::map<std::pair<long, long>, int> task_of;
  std::vector<arslam::CovPairTask> tasks;
  std::vector<int2> rhs;
  std::vector<int> task_rhs;
  size_t panel = 0;   // a panel's doubles
  int batch_panels = 1, per_batch = 1, n_batches = 0;
  // 3. per panel, the tile rows its right-hand sides touch (active), then those its pairs read (needed)
  int all_panels = 0;
  std::vector<unsigned char> mask;
  // 4. the tasks' blocks and statuses as the device left them
  std::vector<double> out;
  std::vector<int> st;
  std::pair<long, long> task_key(int pair) const {
    const long ka = blk[2L * pair].key(), kb = blk[2L * pair + 1].key();
    return std::make_pair(std::min(ka, kb), std::max(ka, kb));
  }
};

namespace {
using PairPlan = arslam_lm::CovPairPlan;

// stage 1, before cov_factor: the caller's blocks in the device problem (BlockMap: per block, under any e-block set)
void pairs_resolve(const std::string &who, const arslam_lm::BlockMap &bm, const arslam_lm_cov_pair *pairs, int n_pairs,
                   PairPlan &pp) {
  const auto device_block = [&](int kind, int index) -> PairPlan::Blk {
    fail_if(kind != ARSLAM_BLOCK_CAMERA && kind != ARSLAM_BLOCK_CAPTURE && kind != ARSLAM_BLOCK_TAG,
            ARSLAM_E_INVALID_ARG, who + ": kind must be ARSLAM_BLOCK_CAMERA, _CAPTURE or _TAG");
    if (kind == ARSLAM_BLOCK_CAMERA) {
      fail_if(index != 0, ARSLAM_E_INVALID_ARG, who + ": the camera's index is 0");
      return PairPlan::Blk{arslam::kCovFocal, 0};
    }
    const bool cap = kind == ARSLAM_BLOCK_CAPTURE;
    fail_if(index < 0 || index >= (cap ? bm.n_cap : bm.n_tag), ARSLAM_E_INVALID_ARG, who + ": block index out of range");
    return PairPlan::Blk{bm.role(cap, index), bm.idx(cap, index)};
  };
  pp.blk.resize(2L * n_pairs);
  for (int i = 0; i < n_pairs; ++i) {
    pp.blk[2L * i] = device_block(pairs[i].kind_a, pairs[i].index_a);
    pp.blk[2L * i + 1] = device_block(pairs[i].kind_b, pairs[i].index_b);
  }
}

// stage 1, after it: a pair is available when both its blocks are free, have rows and are not the call's anchor
void pairs_available(const arslam_lm &h, const arslam_lm::CovFactor &cf, PairPlan &pp) {
  const auto available = [&](const PairPlan::Blk &b) {
    if (b.role == arslam::kCovFocal) return h.has_f && h.P.cam_row >= 0;
    if (cf.is_anchor(b.role, b.idx)) return false;   // (held fixed for this call)
    if (b.role == arslam::kCovF)
      return h.has_f && h.cov_f_free(b.idx) && (size_t)b.idx < h.lay.tag_row.size() && h.lay.tag_row[b.idx] >= 0;
    return h.cov_e_free(b.idx) && cf.cap_start[b.idx + 1] > cf.cap_start[b.idx];
  };
  pp.avail.assign(pp.blk.size() / 2, 0);
  for (size_t i = 0; i < pp.avail.size(); ++i) pp.avail[i] = available(pp.blk[2 * i]) && available(pp.blk[2 * i + 1]);
}

// stage 2: each unordered pair once, the block of the smaller key as the solved
// side; panels per batch: what fits kCovBatchBytes, kCovBatchPanels at most (a
// panel is T x 32 KB).  tests/lm_cov_pairs_ref.py mirrors this rule.
void pairs_tasks(int T, PairPlan &pp) {
  for (size_t i = 0; i < pp.avail.size(); ++i)
    if (pp.avail[i]) pp.task_of.emplace(pp.task_key((int)i), 0);
  long last = -1;
  for (auto &kv : pp.task_of) {
    const PairPlan::Blk b = PairPlan::Blk::of_key(kv.first.first), a = PairPlan::Blk::of_key(kv.first.second);
    if (pp.rhs.empty() || kv.first.first != last) pp.rhs.push_back(make_int2(b.role, b.idx));
    last = kv.first.first;
    kv.second = (int)pp.tasks.size();
    pp.task_rhs.push_back((int)pp.rhs.size() - 1);
    pp.tasks.push_back(arslam::CovPairTask{a.role, a.idx, b.role, b.idx, 0, (int)pp.tasks.size()});
  }
  pp.panel = (size_t)std::max(T, 1) * 4096;
  pp.batch_panels = (int)std::min<size_t>(arslam_lm::kCovBatchPanels,
                                          std::max<size_t>(1, arslam_lm::kCovBatchBytes / (pp.panel * sizeof(double))));
  pp.per_batch = pp.batch_panels * arslam::kCovPanelBlocks;
  for (size_t t = 0; t < pp.tasks.size(); ++t) pp.tasks[t].slot = pp.task_rhs[t] % pp.per_batch;
  pp.n_batches = ((int)pp.rhs.size() + pp.per_batch - 1) / pp.per_batch;
  pp.out.assign(36L * std::max<size_t>(pp.tasks.size(), 1), -1.0);
  pp.st.assign(std::max<size_t>(pp.tasks.size(), 1), 2);
}

// the caller's pairs: its (a, b) as computed or transposed; the focal's 6 values
// first -- the lens forms: the camera's rows (as a) or columns (as b), 3 when live
void pairs_write(const PairPlan &pp, const arslam_lm::CovFactor &cf, bool lens, double *cov, int *status) {
  const int n_camv = cf.live ? 3 : 1;
  for (size_t i = 0; i < pp.avail.size(); ++i) {
    double *c = cov + 36L * i;
    int s = ARSLAM_COV_UNAVAILABLE;
    if (pp.avail[i]) {
      const PairPlan::Blk &ba = pp.blk[2 * i], &bb = pp.blk[2 * i + 1];
      const int t = pp.task_of.at(pp.task_key((int)i));
      s = (cf.deficient || pp.st[t] != 0) ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_OK;
      if (s == ARSLAM_COV_OK) {
        const double *o = pp.out.data() + 36L * t;   // rows: the larger key's block; columns: the smaller's
        const bool as_is = ba.key() >= bb.key();
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
}
}  // namespace

// stage 3 (a problem with a reduced system): the masks, built on the host from
// the e-blocks' local f-blocks (their reduced rows are where an e-block's
// columns and rows live), uploaded; the panels and the batches' events
void arslam_lm::cov_pair_masks(const CovFactor &cf, CovPairPlan &pp) {
  const int T = plan.T, n_rhs = (int)pp.rhs.size(), n_tasks = (int)pp.tasks.size();
  pp.mask.assign(2 * (size_t)pp.all_panels * T, 0);
  unsigned char *active = pp.mask.data(), *needed = pp.mask.data() + (size_t)pp.all_panels * T;
  if (!cov_tp_ready) {
    arslam::tile_solve_plan_build(plan, cov_tp, stream);
    cov_tp_ready = true;
  }
  std::vector<int> h_bs(nc + 1, 0), h_bt;
  bool any_e = false;
  for (const auto &t : pp.tasks) any_e = any_e || t.role_a == arslam::kCovE || t.role_b == arslam::kCovE;
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
      if (cf.live) arslam::tile_solve_mark(cov_tp, m, P.cam_row + 2);
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
  for (int r = 0; r < n_rhs; ++r) mark(active + (size_t)(r / arslam::kCovPanelBlocks) * T, pp.rhs[r].x, pp.rhs[r].y);
  for (int t = 0; t < n_tasks; ++t)
    mark(needed + (size_t)(pp.task_rhs[t] / arslam::kCovPanelBlocks) * T, pp.tasks[t].role_a, pp.tasks[t].idx_a);
  d_pair_mask.alloc(pp.mask.size());
  d_pair_mask.upload(pp.mask.data(), pp.mask.size(), stream);
  d_pair_B.alloc(pp.panel * std::min(pp.batch_panels, pp.all_panels));
  while ((int)pair_ev.size() < 2 * pp.n_batches) {
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreate(&e));
    pair_ev.push_back(e);
  }
}

// stage 4: the distinct solved blocks through the solve in batches, each
// batch's tasks behind it, the results on their way to the host
void arslam_lm::cov_pair_batches(CovFactor &cf, CovPairPlan &pp) {
  const int T = plan.T, n_rhs = (int)pp.rhs.size(), n_tasks = (int)pp.tasks.size();
  const unsigned char *active = pp.mask.data(), *needed = pp.mask.data() + (size_t)pp.all_panels * T;
  d_pair_rhs.alloc(n_rhs);
  d_pair_tasks.alloc(n_tasks);
  d_pair_out.alloc(36L * n_tasks);
  d_pair_status.alloc(n_tasks);
  d_pair_rhs.upload(pp.rhs.data(), n_rhs, stream);
  d_pair_tasks.upload(pp.tasks.data(), n_tasks, stream);
  int t0 = 0;
  for (int bt = 0; bt < pp.n_batches; ++bt) {
    const int r0 = bt * pp.per_batch, nr = std::min(pp.per_batch, n_rhs - r0);
    const int np = (nr + arslam::kCovPanelBlocks - 1) / arslam::kCovPanelBlocks;
    int t1 = t0;
    while (t1 < n_tasks && pp.task_rhs[t1] < r0 + nr) ++t1;
    if (has_f) {
      const size_t m0 = (size_t)bt * pp.batch_panels * T;   // this batch's first panel in the masks
      HIP_CHECK(hipMemsetAsync(d_pair_B.p, 0, pp.panel * np * sizeof(double), stream));
      if (cf.live) arslam::launch_cov_pair_rhs_lens(P, d_cov_Y.p, d_cov_R.p, d_cov_Gl.p, d_pair_rhs.p + r0, nr, d_pair_B.p, stream);
      else arslam::launch_cov_pair_rhs(P, d_cov_Y.p, d_cov_R.p, d_pair_rhs.p + r0, nr, d_pair_B.p, stream);
      HIP_CHECK(hipEventRecord(pair_ev[2 * bt], stream));
      arslam::launch_tile_solve(plan, cov_tp, Sp, nR, d_pair_B.p, np, d_pair_mask.p + m0,
                                d_pair_mask.p + (size_t)pp.all_panels * T + m0, d_flag.p, stream);
      HIP_CHECK(hipEventRecord(pair_ev[2 * bt + 1], stream));
      for (int p = 0; p < np; ++p)
        cf.info.n_selinv_products += arslam::tile_solve_products(plan, cov_tp, active + m0 + (size_t)p * T, needed + m0 + (size_t)p * T);
    }
    if (cf.live)
      arslam::launch_cov_pair_blocks_lens(P, d_pair_B.p, cf.scale, d_cov_Y.p, d_cov_R.p, d_cov_Gl.p, d_pair_tasks.p + t0,
                                          t1 - t0, d_pair_out.p, d_pair_status.p, d_flag.p, stream);
    else
      arslam::launch_cov_pair_blocks(P, has_f ? d_pair_B.p : nullptr, cf.scale, d_cov_Y.p, d_cov_R.p, d_pair_tasks.p + t0,
                                     t1 - t0, d_pair_out.p, d_pair_status.p, d_flag.p, stream);
    t0 = t1;
  }
  HIP_CHECK(hipEventRecord(cov_ev[3], stream));
  HIP_CHECK(hipMemcpyAsync(pp.out.data(), d_pair_out.p, 36L * n_tasks * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(pp.st.data(), d_pair_status.p, n_tasks * sizeof(int), hipMemcpyDeviceToHost, stream));
}

// Cross-covariance blocks of the same matrix (arslam_lm.h): cov_factor, then
// whole columns of Z = S^-1 by the multi-right-hand-side tile solve
// (cov_pairs.hip) on the factor itself -- this call never runs the selected
// inverse, whose first kernel overwrites the off-diagonal factor tiles in
// place, and it refactors every time, so an earlier covariance() leaves it
// nothing to trip over; nor does it touch the kept result.  Each unordered pair
// is computed once, the other order is its transpose (pairs_tasks).  The
// distinct solved blocks go through the solve in batches of at most
// kCovBatchPanels panels and kCovBatchBytes.  A right-hand side is non-zero
// only in the tile rows of its block, so the forward pass touches their
// ancestors in the elimination tree and nothing else, and the backward pass
// computes only the tile rows some pair of the panel reads (and their
// ancestors): per-panel byte masks (cov_pair_masks).
// A lens form: the camera's block is [f, l1, l2]; with l1, l2 live its
// right-hand side is three unit columns and the lens instances of the two small
// kernels run (cov_lens.hip).
void arslam_lm::covariance_pairs(const CovForm &form, const arslam_lm_cov_pair *pairs, int n_pairs, double *cov,
                                 int *status, arslam_lm_cov_info *info_out) {
  const std::string who = form.name("covariance_pairs");
  cov_check_state(who, form);
  const BlockMap bm = block_map();
  cov_check_anchor(who, form, bm);
  CovPairPlan pp;
  pairs_resolve(who, bm, pairs, n_pairs, pp);
  CovFactor cf;
  cov_factor(cf, form, bm);
  pairs_available(*this, cf, pp);
  pairs_tasks(plan.T, pp);
  const bool run = cf.factored && !pp.tasks.empty();
  if (run) {
    pp.all_panels = ((int)pp.rhs.size() + arslam::kCovPanelBlocks - 1) / arslam::kCovPanelBlocks;   // (a batch holds whole panels)
    if (has_f) cov_pair_masks(cf, pp);
    cov_pair_batches(cf, pp);
  }
  cov_numeric_test(cf);
  if (run) {
    float all = 0.f, solve = 0.f;
    HIP_CHECK(hipEventElapsedTime(&all, cov_ev[2], cov_ev[3]));
    for (int bt = 0; has_f && bt < pp.n_batches; ++bt) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, pair_ev[2 * bt], pair_ev[2 * bt + 1]));
      solve += ms;
    }
    cf.info.t_selinv_ms = solve;
    cf.info.t_blocks_ms = std::max(0.f, all - solve);
  }
  pairs_write(pp, cf, form.lens, cov, status);
  if (info_out) *info_out = cf.info;
}
