// host_problem.cpp -- the host structure of a device problem
// (host_structure.h).  Restates the parameter-block bookkeeping of
// ceres::Problem as ar_slam builds it (AddResidualBlock, ar_slam_util.cpp:
// 720-727, 829-836, 956-963; SetParameterBlockConstant, :965, :972) and the
// DENSE_SCHUR split (captures eliminated, tags + camera reduced).
#include "host_structure.h"

#include <algorithm>
#include <cstring>

namespace arslam {

HostProblem host_problem(const arslam_soa_problem *p, const ObsLoss *loss, const arslam_soa_problem *whole) {
  api_check(p != nullptr, ARSLAM_E_INVALID_ARG, "null problem");
  api_check(p->n_cap >= 0 && p->n_tag >= 0 && p->n_obs >= 0, ARSLAM_E_INVALID_ARG, "negative sizes");
  api_check(p->camera && (!p->n_cap || p->cap) && (!p->n_tag || p->tag), ARSLAM_E_INVALID_ARG,
            "null parameter arrays");
  api_check(!p->n_obs || (p->obs_cap && p->obs_tag && p->corners), ARSLAM_E_INVALID_ARG,
            "null observation arrays");
  HostProblem h;
  const int nc = h.nc = p->n_cap, nt = h.nt = p->n_tag, nb = h.nb = p->n_obs;
  const long n = h.n = 3 + 6L * nc + 6L * nt;
  // capture-major observation order (stable)
  h.cap_start.assign(nc + 1, 0);
  for (int b = 0; b < nb; ++b) {
    api_check(p->obs_cap[b] >= 0 && p->obs_cap[b] < nc, ARSLAM_E_INVALID_ARG, "obs_cap out of range");
    api_check(p->obs_tag[b] >= 0 && p->obs_tag[b] < nt, ARSLAM_E_INVALID_ARG, "obs_tag out of range");
    h.cap_start[p->obs_cap[b] + 1]++;
  }
  for (int c = 0; c < nc; ++c) {
    h.maxk = std::max(h.maxk, h.cap_start[c + 1]);
    h.cap_start[c + 1] += h.cap_start[c];
  }
  std::vector<int> order(nb);
  {
    std::vector<int> fill(h.cap_start.begin(), h.cap_start.end() - 1);
    for (int b = 0; b < nb; ++b) order[fill[p->obs_cap[b]]++] = b;
  }
  h.obs_tag.resize(nb);
  h.obs_lblk.resize(nb);
  h.cap_blk_start.assign(nc + 1, 0);
  h.corners.resize(8L * nb);
  h.blk_tag.reserve(nb);
  for (int c = 0; c < nc; ++c) {
    h.cap_blk_start[c] = (int)h.blk_tag.size();
    for (int q = h.cap_start[c]; q < h.cap_start[c + 1]; ++q) {
      const int b = order[q];
      const int t = p->obs_tag[b];
      h.obs_tag[q] = t;
      std::memcpy(&h.corners[8L * q], p->corners + 8L * b, 8 * sizeof(double));
      int u = -1;
      for (int i = h.cap_blk_start[c]; i < (int)h.blk_tag.size(); ++i)
        if (h.blk_tag[i] == t) { u = i - h.cap_blk_start[c]; break; }
      if (u < 0) { u = (int)h.blk_tag.size() - h.cap_blk_start[c]; h.blk_tag.push_back(t); }
      h.obs_lblk[q] = u + 1;
    }
    h.maxblk = std::max(h.maxblk, (int)h.blk_tag.size() - h.cap_blk_start[c]);
  }
  h.cap_blk_start[nc] = (int)h.blk_tag.size();
  // the losses in the same order (kept only when some observation has one)
  bool any_loss = false;
  if (loss && loss->kind && loss->a)
    for (int b = 0; b < nb && !any_loss; ++b) any_loss = loss->kind[b] != ARSLAM_LOSS_NONE;
  if (any_loss) {
    h.loss_kind.resize(nb);
    h.loss_a.resize(nb);
    for (int q = 0; q < nb; ++q) {
      h.loss_kind[q] = loss->kind[order[q]];
      h.loss_a[q] = loss->a[order[q]];
    }
  }
  // the tag sides in the same order (kept only when some side is not the default)
  bool any_size = false;
  if (loss && loss->size)
    for (int b = 0; b < nb && !any_size; ++b) any_size = loss->size[b] != ARSLAM_DEFAULT_TAG_SIZE;
  if (any_size) {
    h.obs_size.resize(nb);
    for (int q = 0; q < nb; ++q) h.obs_size[q] = loss->size[order[q]];
  }
  api_check(h.maxblk <= kMaxSchurBlocks, ARSLAM_E_UNSUPPORTED,
            "an eliminated block (capture, or tag under tag elimination) couples more than 256 distinct blocks");
  // tag CSR over the capture-major order
  h.tag_start.assign(nt + 1, 0);
  h.tag_obs.resize(nb);
  h.obs_tpos.resize(nb);
  for (int q = 0; q < nb; ++q) h.tag_start[h.obs_tag[q] + 1]++;
  for (int t = 0; t < nt; ++t) h.tag_start[t + 1] += h.tag_start[t];
  {
    std::vector<int> fill(h.tag_start.begin(), h.tag_start.end() - 1);
    for (int q = 0; q < nb; ++q) {
      h.obs_tpos[q] = fill[h.obs_tag[q]]++;
      h.tag_obs[h.obs_tpos[q]] = q;
    }
  }
  // free slots (the tags' use and the observation count are the whole problem's)
  const arslam_soa_problem &w = whole ? *whole : *p;
  std::vector<int> tag_deg(nt, 0);
  for (int b = 0; b < w.n_obs; ++b) tag_deg[w.obs_tag[b]]++;
  h.nb_global = w.n_obs;
  h.slot_free.assign(n, 0);
  const bool cam_free = !p->camera_const && h.nb_global > 0;
  for (int j = 0; j < 3; ++j) h.slot_free[j] = cam_free;
  for (int c = 0; c < nc; ++c) {
    const bool f = h.cap_start[c + 1] > h.cap_start[c] && !(p->cap_const && p->cap_const[c]);
    for (int j = 0; j < 6; ++j) h.slot_free[3 + 6L * c + j] = f;
  }
  for (int t = 0; t < nt; ++t) {
    const bool f = tag_deg[t] > 0 && !(p->tag_const && p->tag_const[t]);
    for (int j = 0; j < 6; ++j) h.slot_free[3 + 6L * nc + 6L * t + j] = f;
  }
  h.obs_active.resize(nb);
  for (int q = 0; q < nb; ++q) {
    const int c = p->obs_cap[order[q]];
    h.obs_active[q] = h.slot_free[0] || h.slot_free[3 + 6L * c] || h.slot_free[3 + 6L * nc + 6L * h.obs_tag[q]];
  }
  h.x0.resize(n);
  std::memcpy(h.x0.data(), p->camera, 3 * sizeof(double));
  if (nc) std::memcpy(h.x0.data() + 3, p->cap, 6L * nc * sizeof(double));
  if (nt) std::memcpy(h.x0.data() + 3 + 6L * nc, p->tag, 6L * nt * sizeof(double));
  return h;
}

}  // namespace arslam
