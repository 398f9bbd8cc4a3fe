// host_eblocks.cpp -- which blocks the device eliminates (host_structure.h):
// Ceres 2.0's e-block set for DENSE_SCHUR, and the device problem of a side --
// the problem itself, its role swap, or the mixed regrouping.
#include "host_structure.h"

#include <algorithm>
#include <cstring>

namespace arslam {

// Ceres 2.0 (reorder_program.cc ComputeStableSchurOrdering, graph_algorithms.h
// StableIndependentSetOrdering): vertices are the
// non-constant parameter blocks in program order -- the order in which
// AddResidualBlock(cost, nullptr, camera, capture, tag) first saw them,
// ar_slam_util.cpp:723-727 -- with an edge between every two non-constant
// blocks of one residual.  The vertices are stable-sorted by ascending degree
// and taken greedily: a vertex none of whose neighbours is taken joins the
// independent set (the e-blocks).
SchurSide ceres_schur_side(const arslam_soa_problem *p, std::vector<uint8_t> *e_cap, std::vector<uint8_t> *e_tag) {
  SchurSide out;
  if (e_cap) e_cap->assign(p ? std::max(p->n_cap, 0) : 0, 0);
  if (e_tag) e_tag->assign(p ? std::max(p->n_tag, 0) : 0, 0);
  api_check(p != nullptr, ARSLAM_E_INVALID_ARG, "null problem");
  api_check(p->n_cap >= 0 && p->n_tag >= 0 && p->n_obs >= 0, ARSLAM_E_INVALID_ARG, "negative sizes");
  api_check(!p->n_obs || (p->obs_cap && p->obs_tag), ARSLAM_E_INVALID_ARG, "null observation arrays");
  const int nc = p->n_cap, nt = p->n_tag, nb = p->n_obs;
  for (int b = 0; b < nb; ++b) {
    api_check(p->obs_cap[b] >= 0 && p->obs_cap[b] < nc, ARSLAM_E_INVALID_ARG, "obs_cap out of range");
    api_check(p->obs_tag[b] >= 0 && p->obs_tag[b] < nt, ARSLAM_E_INVALID_ARG, "obs_tag out of range");
  }
  if (nb == 0) return out;
  auto cap_free = [&](int c) { return !(p->cap_const && p->cap_const[c]); };
  auto tag_free = [&](int t) { return !(p->tag_const && p->tag_const[t]); };
  const bool cam_free = !p->camera_const;
  // distinct (capture, tag) pairs of free blocks in both directions, in
  // O(observations): bucketed by capture (a counting sort), duplicates dropped
  // with a last-seen capture per tag (the adjacency lists are sets: their
  // order does not change the independent set)
  std::vector<int> tag_nobs(nt, 0);
  for (int b = 0; b < nb; ++b) out.max_tag_obs = std::max(out.max_tag_obs, ++tag_nobs[p->obs_tag[b]]);
  std::vector<int> by_cap_start(nc + 1, 0), by_cap(nb);
  for (int b = 0; b < nb; ++b) by_cap_start[p->obs_cap[b] + 1]++;
  for (int c = 0; c < nc; ++c) by_cap_start[c + 1] += by_cap_start[c];
  {
    std::vector<int> fill(by_cap_start.begin(), by_cap_start.end() - 1);
    for (int b = 0; b < nb; ++b) by_cap[fill[p->obs_cap[b]]++] = b;
  }
  {   // the most distinct tags of one capture and captures of one tag, constant blocks included
      // (the local system an e-block's k_schur wave holds: kMaxSchurBlocks)
    std::vector<int> last(nt, -1), ncap(nt, 0);
    for (int c = 0; c < nc; ++c) {
      int d = 0;
      for (int q = by_cap_start[c]; q < by_cap_start[c + 1]; ++q) {
        const int t = p->obs_tag[by_cap[q]];
        if (last[t] == c) continue;
        last[t] = c;
        ++d;
        out.max_tag_blk = std::max(out.max_tag_blk, ++ncap[t]);
      }
      out.max_cap_blk = std::max(out.max_cap_blk, d);
    }
  }
  std::vector<int> cap_adj_start(nc + 1, 0), cap_adj, tag_adj_start(nt + 1, 0), mark(nt, -1);
  cap_adj.reserve(nb);
  for (int c = 0; c < nc; ++c) {
    if (cap_free(c))
      for (int q = by_cap_start[c]; q < by_cap_start[c + 1]; ++q) {
        const int t = p->obs_tag[by_cap[q]];
        if (!tag_free(t) || mark[t] == c) continue;
        mark[t] = c;
        cap_adj.push_back(t);
        tag_adj_start[t + 1]++;
      }
    cap_adj_start[c + 1] = (int)cap_adj.size();
  }
  for (int t = 0; t < nt; ++t) tag_adj_start[t + 1] += tag_adj_start[t];
  std::vector<int> tag_adj(tag_adj_start[nt]);
  {
    std::vector<int> ft(tag_adj_start.begin(), tag_adj_start.end() - 1);
    for (int c = 0; c < nc; ++c)
      for (int q = cap_adj_start[c]; q < cap_adj_start[c + 1]; ++q) tag_adj[ft[cap_adj[q]]++] = c;
  }
  // vertex ids: 0 camera, 1 + c capture, 1 + nc + t tag; program order
  const int nv = 1 + nc + nt;
  std::vector<int> order;
  order.reserve(nv);
  std::vector<char> seen(nv, 0);
  auto visit = [&](int v, bool free_) {
    if (free_ && !seen[v]) { seen[v] = 1; order.push_back(v); }
  };
  for (int b = 0; b < nb; ++b) {
    visit(0, cam_free);
    visit(1 + p->obs_cap[b], cap_free(p->obs_cap[b]));
    visit(1 + nc + p->obs_tag[b], tag_free(p->obs_tag[b]));
  }
  const int cam_deg = (int)order.size() - (cam_free ? 1 : 0);
  auto degree = [&](int v) {
    if (v == 0) return cam_deg;
    if (v <= nc) return cap_adj_start[v] - cap_adj_start[v - 1] + (cam_free ? 1 : 0);
    const int t = v - 1 - nc;
    return tag_adj_start[t + 1] - tag_adj_start[t] + (cam_free ? 1 : 0);
  };
  std::vector<int> deg(nv, 0);
  int max_deg = 0;
  for (int v : order) max_deg = std::max(max_deg, deg[v] = degree(v));
  {   // stable sort by ascending degree: a counting sort
    std::vector<int> cnt(max_deg + 2, 0), sorted(order.size());
    for (int v : order) cnt[deg[v] + 1]++;
    for (int d = 0; d <= max_deg; ++d) cnt[d + 1] += cnt[d];
    for (int v : order) sorted[cnt[deg[v]]++] = v;
    order.swap(sorted);
  }
  enum : char { kWhite = 0, kGrey = 1, kBlack = 2 };
  std::vector<char> color(nv, kWhite);
  for (int v : order) {
    if (color[v] != kWhite) continue;
    color[v] = kBlack;
    if (v == 0) {
      ++out.e_cam;
      for (int u : order) if (u != 0 && color[u] == kWhite) color[u] = kGrey;   // every block shares a residual with it
      continue;
    }
    if (cam_free && color[0] == kWhite) color[0] = kGrey;
    if (v <= nc) {
      ++out.e_cap;
      if (e_cap) (*e_cap)[v - 1] = 1;
      for (int q = cap_adj_start[v - 1]; q < cap_adj_start[v]; ++q) {
        const int u = 1 + nc + cap_adj[q];
        if (color[u] == kWhite) color[u] = kGrey;
      }
    } else {
      ++out.e_tag;
      const int t = v - 1 - nc;
      if (e_tag) (*e_tag)[t] = 1;
      for (int q = tag_adj_start[t]; q < tag_adj_start[t + 1]; ++q) {
        const int u = 1 + tag_adj[q];
        if (color[u] == kWhite) color[u] = kGrey;
      }
    }
  }
  return out;
}

arslam_soa_problem swap_roles(const arslam_soa_problem &p) {
  arslam_soa_problem s = p;
  s.n_cap = p.n_tag; s.n_tag = p.n_cap;
  s.cap = p.tag; s.tag = p.cap;
  s.obs_cap = p.obs_tag; s.obs_tag = p.obs_cap;
  s.cap_const = p.tag_const; s.tag_const = p.cap_const;
  return s;
}

MixedProblem mixed_problem(const arslam_soa_problem &p, const std::vector<uint8_t> &e_cap,
                           const std::vector<uint8_t> &e_tag) {
  MixedProblem m;
  const int nc = p.n_cap, nt = p.n_tag, nb = p.n_obs;
  m.src_n_cap = nc;
  m.src_n_tag = nt;
  std::vector<int> cap_f(nc, -1), tag_f(nt, -1), cap_g(nc, -1), tag_g(nt, -1), cap_d(nc, -1);
  for (int t = 0; t < nt; ++t)
    if (!e_tag[t]) { tag_f[t] = (int)m.f_src.size(); m.f_src.push_back(t); m.f_is_cap.push_back(0); }
  for (int c = 0; c < nc; ++c)
    if (!e_cap[c]) { cap_f[c] = (int)m.f_src.size(); m.f_src.push_back(c); m.f_is_cap.push_back(1); }
  for (int c = 0; c < nc; ++c)
    if (e_cap[c]) { cap_g[c] = (int)m.kind.size(); m.kind.push_back(kMixCap); m.group_src.push_back(c); }
  for (int t = 0; t < nt; ++t)
    if (e_tag[t]) { tag_g[t] = (int)m.kind.size(); m.kind.push_back(kMixTag); m.group_src.push_back(t); }
  for (int b = 0; b < nb; ++b) {
    const int c = p.obs_cap[b], t = p.obs_tag[b];
    api_check(!(e_cap[c] && e_tag[t]), ARSLAM_E_INVALID_ARG, "mixed e-set: a residual joins two e-blocks");
    if (!e_cap[c] && !e_tag[t] && cap_d[c] < 0) {
      cap_d[c] = (int)m.kind.size();
      m.kind.push_back(kMixDirect);
      m.group_src.push_back(c);
    }
  }
  const int ng = (int)m.kind.size(), nf = (int)m.f_src.size();
  m.f_alias.assign(nf, -1);
  for (int c = 0; c < nc; ++c)
    if (cap_d[c] >= 0) { m.f_alias[cap_f[c]] = cap_d[c]; ++m.n_direct; }
  m.obs_cap.resize(nb);
  m.obs_tag.resize(nb);
  for (int b = 0; b < nb; ++b) {
    const int c = p.obs_cap[b], t = p.obs_tag[b];
    if (e_cap[c]) { m.obs_cap[b] = cap_g[c]; m.obs_tag[b] = tag_f[t]; }
    else if (e_tag[t]) { m.obs_cap[b] = tag_g[t]; m.obs_tag[b] = cap_f[c]; }
    else { m.obs_cap[b] = cap_d[c]; m.obs_tag[b] = tag_f[t]; }
  }
  m.cap.resize(6L * ng);
  m.tag.resize(6L * nf);
  m.cap_const.resize(ng);
  m.tag_const.resize(nf);
  for (int g = 0; g < ng; ++g) {
    const bool is_tag = m.kind[g] == kMixTag;
    const unsigned char *cst = is_tag ? p.tag_const : p.cap_const;
    m.cap_const[g] = cst ? cst[m.group_src[g]] : 0;
  }
  for (int f = 0; f < nf; ++f) {
    const unsigned char *cst = m.f_is_cap[f] ? p.cap_const : p.tag_const;
    m.tag_const[f] = cst ? cst[m.f_src[f]] : 0;
  }
  m.soa = p;
  m.soa.n_cap = ng;
  m.soa.n_tag = nf;
  m.soa.cap = m.cap.data();
  m.soa.tag = m.tag.data();
  m.soa.obs_cap = m.obs_cap.data();
  m.soa.obs_tag = m.obs_tag.data();
  m.soa.cap_const = m.cap_const.data();
  m.soa.tag_const = m.tag_const.data();
  std::vector<double> x(3 + 6L * ng + 6L * nf);
  mixed_values(m, p, x.data());
  if (ng) std::memcpy(m.cap.data(), x.data() + 3, 6L * ng * sizeof(double));
  if (nf) std::memcpy(m.tag.data(), x.data() + 3 + 6L * ng, 6L * nf * sizeof(double));
  return m;
}

void mixed_values(const MixedProblem &m, const arslam_soa_problem &p, double *x) {
  const long ng = (long)m.kind.size(), nf = (long)m.f_src.size();
  std::memcpy(x, p.camera, 3 * sizeof(double));
  for (long g = 0; g < ng; ++g) {
    const double *src = m.kind[g] == kMixTag ? p.tag : p.cap;
    std::memcpy(x + 3 + 6 * g, src + 6L * m.group_src[g], 6 * sizeof(double));
  }
  for (long f = 0; f < nf; ++f) {
    const double *src = m.f_is_cap[f] ? p.cap : p.tag;
    std::memcpy(x + 3 + 6 * ng + 6 * f, src + 6L * m.f_src[f], 6 * sizeof(double));
  }
}

void mixed_patch(HostProblem &h, const MixedProblem &m, const arslam_soa_problem &p) {
  const int ng = h.nc, nf = h.nt;
  // the direct groups' own f-block, last in their block lists
  std::vector<int> own(ng, -1);
  for (int f = 0; f < nf; ++f)
    if (m.f_alias[f] >= 0) own[m.f_alias[f]] = f;
  std::vector<int> start(ng + 1, 0), blk;
  blk.reserve(h.blk_tag.size() + m.n_direct);
  h.maxblk = 0;
  for (int g = 0; g < ng; ++g) {
    start[g] = (int)blk.size();
    blk.insert(blk.end(), h.blk_tag.begin() + h.cap_blk_start[g], h.blk_tag.begin() + h.cap_blk_start[g + 1]);
    if (own[g] >= 0) blk.push_back(own[g]);
    h.maxblk = std::max(h.maxblk, (int)blk.size() - start[g]);
  }
  start[ng] = (int)blk.size();
  h.cap_blk_start.swap(start);
  h.blk_tag.swap(blk);
  api_check(h.maxblk <= kMaxSchurBlocks, ARSLAM_E_UNSUPPORTED,
            "an eliminated block (or a direct group) couples more than 256 distinct blocks");
  // an f-block is free iff its original block is (a capture on the reduced side
  // may be used only by residuals of its own direct group)
  std::vector<char> used_c(p.n_cap, 0), used_t(p.n_tag, 0);
  for (int b = 0; b < p.n_obs; ++b) { used_c[p.obs_cap[b]] = 1; used_t[p.obs_tag[b]] = 1; }
  for (int f = 0; f < nf; ++f) {
    const int o = m.f_src[f];
    const bool fr = (m.f_is_cap[f] ? used_c[o] : used_t[o]) && !m.tag_const[f];
    for (int j = 0; j < 6; ++j) h.slot_free[3 + 6L * ng + 6L * f + j] = fr;
  }
  // the f-blocks' places for the ordering: a tag's translation; a capture's
  // the mean translation of the tags it sees (its own translation is minus the
  // camera centre, a mirror image of the tags' frame)
  std::vector<double> cap_xyz(3L * p.n_cap, 0.0);
  std::vector<int> cap_n(p.n_cap, 0);
  for (int b = 0; b < p.n_obs; ++b) {
    const int c = p.obs_cap[b];
    for (int a = 0; a < 3; ++a) cap_xyz[3L * c + a] += p.tag[6L * p.obs_tag[b] + a];
    cap_n[c]++;
  }
  h.nd_xyz.assign(3L * nf, 0.0);
  for (int f = 0; f < nf; ++f) {
    const int o = m.f_src[f];
    for (int a = 0; a < 3; ++a)
      h.nd_xyz[3L * f + a] = m.f_is_cap[f] ? (cap_n[o] ? cap_xyz[3L * o + a] / cap_n[o] : 0.0) : p.tag[6L * o + a];
  }
}

const arslam_soa_problem *device_problem(const arslam_soa_problem &p, int side, const std::vector<uint8_t> &e_cap,
                                         const std::vector<uint8_t> &e_tag, arslam_soa_problem &swapped,
                                         MixedProblem &mx) {
  swapped = swap_roles(p);
  mx = side == ARSLAM_ELIM_MIXED ? mixed_problem(p, e_cap, e_tag) : MixedProblem{};
  return side == ARSLAM_ELIM_TAGS ? &swapped : side == ARSLAM_ELIM_MIXED ? &mx.soa : &p;
}

HostProblem device_host_problem(const arslam_soa_problem *dev, const MixedProblem *mx, const arslam_soa_problem &p,
                                const ObsLoss *loss) {
  HostProblem h = host_problem(dev, loss);   // validates dev
  if (mx) mixed_patch(h, *mx, p);
  return h;
}

}  // namespace arslam
