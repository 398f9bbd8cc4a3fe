// host_layout.cpp -- the reduced system's row layout and tile pattern, and the
// memory of the elimination order between loads (host_structure.h).
#include "host_structure.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iterator>

namespace arslam {

double scalar_cholesky_flops(const std::vector<std::vector<int>> &adj, const std::vector<int> &tag_row,
                             bool camera) {
  // tags in elimination order; symbolic factorization on the tag graph: the
  // higher-ordered neighbour set of a tag (its fill included) is merged into
  // its elimination-tree parent, the lowest of them
  std::vector<int> order;
  for (int t = 0; t < (int)tag_row.size(); ++t)
    if (tag_row[t] >= 0) order.push_back(t);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return tag_row[a] < tag_row[b]; });
  std::vector<int> pos(tag_row.size(), -1);
  for (int i = 0; i < (int)order.size(); ++i) pos[order[i]] = i;
  const int n = (int)order.size();
  std::vector<std::vector<int>> up(n);   // higher-ordered neighbours (positions), sorted
  for (int i = 0; i < n; ++i) {
    for (int v : adj[order[i]])
      if (v < (int)pos.size() && pos[v] > i) up[i].push_back(pos[v]);
    std::sort(up[i].begin(), up[i].end());
    up[i].erase(std::unique(up[i].begin(), up[i].end()), up[i].end());
  }
  const double ncam = camera ? 3.0 : 0.0;
  double flops = 0.0;
  auto col = [&](double c) { flops += c * (c + 1.0) + c + 1.0; };
  std::vector<int> merged;
  for (int i = 0; i < n; ++i) {
    const double f = (double)up[i].size();
    for (int k = 0; k < 6; ++k) col((5 - k) + 6.0 * f + ncam);
    if (!up[i].empty()) {
      const int parent = up[i][0];
      merged.clear();
      std::set_union(up[parent].begin(), up[parent].end(), up[i].begin() + 1, up[i].end(),
                     std::back_inserter(merged));
      up[parent].swap(merged);
    }
    std::vector<int>().swap(up[i]);
  }
  for (int k = 0; k < (int)ncam; ++k) col(ncam - 1 - k);
  return flops;
}

namespace {

double clock_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The co-visibility graph of the free tags: per tag, the distinct free tags
// of the captures whose blocks list it, ascending (a stamp array dedupes them
// before the sort: the pairs repeat in every capture that sees both; a mixed
// set's direct group lists its own pose, which no residual of the group has as
// its tag).  (Also for the natural order: the scalar flop count reads it.)
std::vector<std::vector<int>> tag_adjacency(const HostProblem &h, const std::vector<char> &tfree) {
  const int nc = h.nc, nt = h.nt;
  std::vector<std::vector<int>> adj(nt);
  if (nt <= 1) return adj;
  std::vector<int> tcap_start(nt + 1, 0), tcap(h.blk_tag.size());
  for (int t : h.blk_tag) tcap_start[t + 1]++;
  for (int t = 0; t < nt; ++t) tcap_start[t + 1] += tcap_start[t];
  {
    std::vector<int> fill(tcap_start.begin(), tcap_start.end() - 1);
    for (int c = 0; c < nc; ++c)
      for (int bb = h.cap_blk_start[c]; bb < h.cap_blk_start[c + 1]; ++bb) tcap[fill[h.blk_tag[bb]]++] = c;
  }
  std::vector<int> stamp(nt, -1);
  for (int a = 0; a < nt; ++a) {
    if (!tfree[a]) continue;
    std::vector<int> &v = adj[a];
    for (int q = tcap_start[a]; q < tcap_start[a + 1]; ++q) {
      const int c = tcap[q];
      for (int bb = h.cap_blk_start[c]; bb < h.cap_blk_start[c + 1]; ++bb) {
        const int b = h.blk_tag[bb];
        if (b != a && tfree[b] && stamp[b] != a) {
          stamp[b] = a;
          v.push_back(b);
        }
      }
    }
    std::sort(v.begin(), v.end());
  }
  return adj;
}

// The order decision: are the request's rows kept?  They must cover no more
// blocks than h has (by identity: exactly h's), the graph must not have
// outgrown them, and (by index) the same blocks must be free.
bool keeps_order(const LayoutRequest &rq, const std::vector<char> &tfree, long n_edges) {
  if (!rq.reuse_rows) return false;
  const std::vector<int> &rows = *rq.reuse_rows;
  const int nt = (int)tfree.size();
  if ((int)rows.size() > std::max(nt, 1) || OrderMemory::graph_outgrown(n_edges, rq.reuse_edges)) return false;
  if (rq.by_identity) return (int)rows.size() == nt;
  for (int t = 0; t < std::min((int)rows.size(), nt); ++t)
    if ((rows[t] >= 0) != (tfree[t] != 0)) return false;
  return true;
}

// A fresh order's parts, in elimination order: one part (natural, RCM) or
// nested dissection's leaves and separators.
std::vector<std::vector<int>> fresh_parts(const HostProblem &h, const std::vector<std::vector<int>> &adj,
                                          const LayoutRequest &rq) {
  const int nc = h.nc, nt = h.nt;
  if (rq.ordering == 2 && nt > 1) {
    // tag positions (initial values) embed the co-visibility graph for geometric separators
    std::vector<double> xyz(3L * nt);
    for (int t = 0; t < nt; ++t)
      for (int a = 0; a < 3; ++a)
        xyz[3L * t + a] = h.nd_xyz.empty() ? h.x0[3 + 6L * nc + 6L * t + a] : h.nd_xyz[3L * t + a];
    // leaves of up to 32 tags (192 rows = 3 whole tiles): a smaller dissection
    // would not shorten the elimination tree, only add padding and parts
    // (debug sweeps; clamped to [1, 4096])
    static const int leaf =
        std::getenv("ARSLAM_ND_LEAF") ? std::min(4096, std::max(1, std::atoi(std::getenv("ARSLAM_ND_LEAF")))) : 32;
    return nd_parts(nt, adj, leaf, xyz, rq.fast_order);
  }
  std::vector<int> order;
  if (rq.ordering == 1 && nt > 1) order = rcm_order(nt, adj);
  else for (int t = 0; t < nt; ++t) order.push_back(t);
  return {order};
}

// Rows exist only for free tags and a free camera (constant / unused blocks
// are not parameters).  kept: the earlier rows, the tags new since (or, by
// identity, new to the reduced side) after them.  Else the parts in order;
// with nested dissection every part starts on a tile boundary so the tile
// elimination tree follows the dissection tree.  The camera's rows come last.
void assign_rows(const HostProblem &h, const std::vector<char> &tfree, const LayoutRequest &rq, bool kept,
                 const std::vector<std::vector<int>> &parts, ReducedLayout &L) {
  const int nc = h.nc, nt = h.nt;
  long row = 0, real = 0;
  if (kept) {
    // (by identity: a tag whose earlier row is no longer a parameter leaves
    // those rows as padding, identity rows like the alignment padding)
    const int n_old = std::min((int)rq.reuse_rows->size(), nt);
    for (int t = 0; t < n_old; ++t) L.tag_row[t] = tfree[t] ? (*rq.reuse_rows)[t] : -1;
    for (int t = 0; t < n_old; ++t)
      if (L.tag_row[t] >= 0) {
        row = std::max(row, (long)L.tag_row[t] + 6);
        real += 6;
      }
    // the tags new since the order was made, at the end of its last part (the
    // root separator): a valid order whatever they couple to, since every
    // part's elimination path ends there; OrderMemory::layout recomputes the
    // order once the tile elimination tree grows taller than a fresh one
    for (int t = 0; t < nt; ++t)
      if (tfree[t] && (t >= n_old || L.tag_row[t] < 0)) {
        L.tag_row[t] = (int)row;
        row += 6;
        real += 6;
      }
  }
  for (auto &part : parts) {
    bool any = false;
    for (int t : part) any = any || tfree[t];
    if (!any) continue;
    L.n_parts++;
    if (rq.ordering == 2) row = round_up(row, kTileRows);
    for (int t : part) {
      if (!tfree[t]) continue;
      L.tag_row[t] = (int)row;
      row += 6;
      real += 6;
    }
  }
  L.pad_rows = row - real;
  L.row_slot.assign(row, -1);
  for (int t = 0; t < nt; ++t)
    if (L.tag_row[t] >= 0)
      for (int j = 0; j < 6; ++j) L.row_slot[L.tag_row[t] + j] = (int)(3 + 6L * nc + 6L * t + j);
  if (h.slot_free[0]) {
    L.cam_row = (int)row;
    for (int j = 0; j < 3; ++j) L.row_slot.push_back(j);
    row += 3;
  }
  L.nR = row;
}

// The lower tile pattern of the assembled system: every group's tiles
// pairwise, and the rhs row's tile row.  (L.N, L.T set; nR > 0)
void tile_pattern(const HostProblem &h, ReducedLayout &L) {
  const int T = L.T;
  std::vector<int> ts;
  for (int c = 0; c < h.nc; ++c) {
    ts.clear();
    group_tiles(h, L.tag_row, L.cam_row, c, ts);
    std::sort(ts.begin(), ts.end());
    ts.erase(std::unique(ts.begin(), ts.end()), ts.end());
    for (size_t a = 0; a < ts.size(); ++a)
      for (size_t b = 0; b <= a; ++b) L.pattern[(size_t)ts[a] * T + ts[b]] = 1;
  }
  const int rhs = (int)(L.nR / kTileRows);
  for (int j = 0; j <= rhs; ++j) L.pattern[(size_t)rhs * T + j] = 1;
}

}  // namespace

void group_tiles(const HostProblem &h, const std::vector<int> &tag_row, int cam_row, int c, std::vector<int> &out) {
  if (cam_row >= 0) {
    out.push_back(cam_row / kTileRows);
    out.push_back((cam_row + 2) / kTileRows);
  }
  for (int a = h.cap_blk_start[c]; a < h.cap_blk_start[c + 1]; ++a) {
    const int r0 = tag_row[h.blk_tag[a]];
    if (r0 < 0) continue;
    out.push_back(r0 / kTileRows);
    out.push_back((r0 + 5) / kTileRows);
  }
}

ReducedLayout reduced_layout(const HostProblem &h, const LayoutRequest &rq) {
  static const bool prof = std::getenv("ARSLAM_SETUP_PROFILE") != nullptr;   // debug: layout phases
  double tl[4] = {prof ? clock_ms() : 0.0, 0, 0, 0};
  const int nt = h.nt;
  ReducedLayout L;
  L.tag_row.assign(std::max(nt, 1), -1);
  std::vector<char> tfree(nt, 0);
  for (int t = 0; t < nt; ++t) tfree[t] = h.slot_free[3 + 6L * h.nc + 6L * t];
  const std::vector<std::vector<int>> adj = tag_adjacency(h, tfree);
  for (auto &v : adj) L.n_edges += (long)v.size();
  if (prof) tl[1] = clock_ms();
  L.order_reused = keeps_order(rq, tfree, L.n_edges);
  L.order_edges = L.order_reused ? rq.reuse_edges : L.n_edges;
  assign_rows(h, tfree, rq, L.order_reused,
              L.order_reused ? std::vector<std::vector<int>>{} : fresh_parts(h, adj, rq), L);
  if (prof) tl[2] = clock_ms();
  L.scalar_flops = scalar_cholesky_flops(adj, L.tag_row, L.cam_row >= 0);
  if (prof) tl[3] = clock_ms();
  if (L.nR == 0) return L;
  L.N = round_up(L.nR + 1, kTileRows);
  const int T = L.T = (int)(L.N / kTileRows);
  L.pattern.assign((size_t)T * T, 0);
  if (!rq.sparse) {
    for (int i = 0; i < T; ++i)
      for (int j = 0; j <= i; ++j) L.pattern[(size_t)i * T + j] = 1;
    return L;
  }
  tile_pattern(h, L);
  if (prof)
    std::fprintf(stderr, "arslam layout: adj %.3f order %.3f flops %.3f pattern %.3f ms\n", tl[1] - tl[0],
                 tl[2] - tl[1], tl[3] - tl[2], clock_ms() - tl[3]);
  return L;
}

void tile_fill(int T, std::vector<uint8_t> &P, std::vector<int> &parent) {
  std::vector<int> rows;
  for (int k = 0; k < T; ++k) {
    P[(long)k * T + k] = 1;
    rows.clear();
    for (int i = k + 1; i < T; ++i)
      if (P[(long)i * T + k]) rows.push_back(i);
    for (size_t a = 0; a < rows.size(); ++a)
      for (size_t b = 0; b <= a; ++b) P[(long)rows[a] * T + rows[b]] = 1;
  }
  parent.assign(T, -1);
  for (int k = 0; k < T; ++k)
    for (int i = k + 1; i < T; ++i)
      if (P[(long)i * T + k]) { parent[k] = i; break; }
}

int etree_height(const ReducedLayout &L) {
  std::vector<uint8_t> P = L.pattern;
  std::vector<int> parent;
  tile_fill(L.T, P, parent);
  std::vector<int> lev(L.T, 1);
  int h = 0;
  for (int k = 0; k < L.T; ++k) {   // (parents have larger indices)
    if (parent[k] >= 0) lev[parent[k]] = std::max(lev[parent[k]], lev[k] + 1);
    h = std::max(h, lev[k]);
  }
  return h;
}

// ---- the order memory ----

void OrderMemory::forget() {
  rows_.clear();
  tag_rows_.clear();
  cap_rows_.clear();
}

LayoutRequest OrderMemory::request(bool reuse, int side, const MixedProblem *mx, int ordering, bool sparse,
                                   int n_groups) {
  LayoutRequest rq;
  rq.ordering = ordering;
  rq.sparse = sparse;
  // (the f-side changed: no order to reuse; a mixed set numbers its reduced
  // blocks anew at every load: none by index)
  const bool was_mixed = side_ == ARSLAM_ELIM_MIXED;
  if (side != side_) forget();
  side_ = side;
  if (mx) {
    rows_.clear();
    if (was_mixed && reuse && !mx->f_src.empty() && (!tag_rows_.empty() || !cap_rows_.empty())) {
      rq.by_identity = true;
      rows_.assign(mx->f_src.size(), -1);
      for (size_t f = 0; f < mx->f_src.size(); ++f) {
        const std::vector<int> &m = mx->f_is_cap[f] ? cap_rows_ : tag_rows_;
        if (mx->f_src[f] < (int)m.size()) rows_[f] = m[mx->f_src[f]];
      }
    }
  }
  if (reuse && !rows_.empty() && ordering_ == ordering && sparse_ == sparse &&
      !groups_outgrown(n_groups, order_groups_)) {
    rq.reuse_rows = &rows_;
    rq.reuse_edges = order_edges_;
  }
  return rq;
}

ReducedLayout OrderMemory::layout(const HostProblem &h, const LayoutRequest &rq, bool *recomputed) const {
  ReducedLayout L = reduced_layout(h, rq);
  const bool too_tall = L.order_reused && L.nR > 0 && etree_height(L) > order_height_ + kHeightSlack;
  if (too_tall) {
    LayoutRequest fresh;
    fresh.ordering = rq.ordering;
    fresh.sparse = rq.sparse;
    fresh.fast_order = true;   // (a grown pointer-keyed problem, as every reuse is)
    L = reduced_layout(h, fresh);
  }
  if (recomputed) *recomputed = too_tall;
  return L;
}

void OrderMemory::remember(const ReducedLayout &L, const HostProblem &h, const LayoutRequest &rq,
                           const MixedProblem *mx) {
  last_reused = L.order_reused;
  if (!L.order_reused) {
    order_groups_ = h.nc;
    order_height_ = L.nR > 0 ? etree_height(L) : 0;
  }
  rows_ = L.tag_row;
  order_edges_ = L.order_edges;
  tag_rows_.clear();
  cap_rows_.clear();
  if (mx) {
    tag_rows_.assign(mx->src_n_tag, -1);
    cap_rows_.assign(mx->src_n_cap, -1);
    for (size_t f = 0; f < mx->f_src.size(); ++f)
      (mx->f_is_cap[f] ? cap_rows_ : tag_rows_)[mx->f_src[f]] = L.tag_row[f];
  }
  ordering_ = rq.ordering;
  sparse_ = rq.sparse;
}

void OrderMemory::graph_build(const HostProblem &h, const ReducedLayout &L) {
  covis_nt_ = h.nt <= 16384 ? h.nt : 0;   // (a 32 MB bit matrix at most; past it only the group rule holds)
  covis_edges_ = 0;
  covis_.assign(((size_t)covis_nt_ * covis_nt_ + 63) / 64, 0);
  for (int c = 0; c < h.nc && covis_nt_; ++c) graph_add(h, L, c);
}

void OrderMemory::graph_add(const HostProblem &h, const ReducedLayout &L, int c) {
  if (!covis_nt_) return;
  for (int a = h.cap_blk_start[c]; a < h.cap_blk_start[c + 1]; ++a)
    for (int b = h.cap_blk_start[c]; b < h.cap_blk_start[c + 1]; ++b) {
      const int ta = h.blk_tag[a], tb = h.blk_tag[b];
      if (ta == tb || L.tag_row[ta] < 0 || L.tag_row[tb] < 0) continue;
      const size_t bit = (size_t)ta * covis_nt_ + tb;
      if (!(covis_[bit >> 6] >> (bit & 63) & 1)) {
        covis_[bit >> 6] |= 1ull << (bit & 63);
        ++covis_edges_;
      }
    }
}

void OrderMemory::add_groups(const HostProblem &h, const ReducedLayout &L, const std::vector<int> &groups) {
  for (int c : groups) graph_add(h, L, c);
}

bool OrderMemory::outgrown(int n_groups) const {
  if (covis_nt_ && graph_outgrown(covis_edges_, order_edges_)) return true;
  return groups_outgrown(n_groups, order_groups_);
}

}  // namespace arslam
