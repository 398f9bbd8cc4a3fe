// host_ordering.cpp -- the elimination orders of the reduced system's tag
// graph (host_structure.h): reverse Cuthill-McKee, and nested dissection with
// geometric and BFS-level separators.
#include "host_structure.h"
#include "host_threads.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>

namespace arslam {

namespace {

// BFS over `mark == tag` nodes from start; fills level of each visited node
// (-1 unvisited) and returns the visit order.
std::vector<int> bfs(int start, const std::vector<std::vector<int>> &adj, const std::vector<int> &mark,
                     int tag, std::vector<int> &lev) {
  std::vector<int> order{start};
  lev[start] = 0;
  for (size_t h = 0; h < order.size(); ++h) {
    const int u = order[h];
    for (int v : adj[u])
      if (mark[v] == tag && lev[v] < 0) {
        lev[v] = lev[u] + 1;
        order.push_back(v);
      }
  }
  return order;
}

// pseudo-peripheral node of the component of `start` (George-Liu)
int peripheral(int start, const std::vector<std::vector<int>> &adj, const std::vector<int> &mark,
               int tag, std::vector<int> &lev) {
  int best = start, depth = -1;
  for (int it = 0; it < 6; ++it) {
    const std::vector<int> ord = bfs(best, adj, mark, tag, lev);
    const int d = lev[ord.back()];
    int far = ord.back();
    for (int u : ord)   // among the last level, the one of least degree
      if (lev[u] == d && adj[u].size() < adj[far].size()) far = u;
    for (int u : ord) lev[u] = -1;
    if (d <= depth) break;
    depth = d;
    best = far;
  }
  return best;
}

double nd_beta() {
  // (debug sweeps; clamped to [0, 4]: a finite, non-negative weight)
  static const double b = std::getenv("ARSLAM_ND_BETA")
                              ? std::min(4.0, std::max(0.0, std::atof(std::getenv("ARSLAM_ND_BETA")) + 0.0))
                              : 0.3;
  return b;
}

// The geometric cuts' quantile window [q, 1 - q] and the smaller side's
// least share of the component (debug sweeps; clamped to [0.05, 0.45] and
// [0, 0.45]).
double nd_env(const char *name, double dflt, double lo, double hi) {
  const char *e = std::getenv(name);
  return e ? std::min(hi, std::max(lo, std::atof(e) + 0.0)) : dflt;
}
double nd_qlo() {
  static const double q = nd_env("ARSLAM_ND_QLO", 0.3, 0.05, 0.45);
  return q;
}
double nd_min_side() {
  static const double f = nd_env("ARSLAM_ND_MIN_SIDE", 0.2, 0.0, 0.45);
  return f;
}

// Elimination-tree height, in tile columns, of a dissection step: the
// separator's tiles plus the larger child's height, which grows about as
// sqrt(size) on these planar co-visibility graphs (cfg3: ~1 tile column per
// sqrt(tag) at the root); balance only breaks ties.
double height_score(long ssz, long na, long nb) {
  return std::ceil(6.0 * ssz / kTileRows) + nd_beta() * std::sqrt((double)std::max(na, nb)) +
         1e-6 * std::labs(na - nb);
}

// The two sides of a separator are dissected concurrently (host_fork2) and
// the directions of a geometric cut searched concurrently: the per-node arrays
// (mark, lev) are shared, but a branch only writes its own nodes and reads
// those and its separator's (the sides are not adjacent), and the parts come
// back in the serial order (side A's, side B's, then the separator).
struct Dissector {
  const std::vector<std::vector<int>> &adj;
  const std::vector<double> &xyz;   // optional 3-D embedding (tag positions), 3 per node
  int leaf;
  bool fast = false;
  std::vector<int> mark, lev;
  std::atomic<int> next_tag{1};

  Dissector(const std::vector<std::vector<int>> &a, const std::vector<double> &coords, int leaf_size)
      : adj(a), xyz(coords), leaf(leaf_size), mark(a.size(), 0), lev(a.size(), -1) {}

  // nodes: all with mark == tag; their parts appended to `parts` in elimination order
  void run(std::vector<int> nodes, int tag, std::vector<std::vector<int>> &parts) {
    if (nodes.empty()) return;
    // split into connected components
    std::vector<std::vector<int>> comps;
    for (int u : nodes) {
      if (lev[u] >= 0) continue;
      std::vector<int> c = bfs(u, adj, mark, tag, lev);
      comps.push_back(std::move(c));
    }
    for (int u : nodes) lev[u] = -1;
    for (auto &c : comps) dissect(c, tag, parts);
  }

  // BFS-level separator: the level that balances the two sides
  bool level_separator(std::vector<int> &comp, int tag, std::vector<int> &A, std::vector<int> &B,
                       std::vector<int> &S) {
    const int s = peripheral(comp[0], adj, mark, tag, lev);
    std::vector<int> ord = bfs(s, adj, mark, tag, lev);
    const int depth = lev[ord.back()];
    if (depth < 2) {
      for (int u : ord) lev[u] = -1;
      return false;
    }
    std::vector<int> cnt(depth + 1, 0);
    for (int u : ord) cnt[lev[u]]++;
    int sep = 1, acc = cnt[0];
    const int half = (int)ord.size() / 2;
    while (sep < depth - 1 && acc + cnt[sep] / 2 < half) acc += cnt[sep++];
    for (int u : ord) {
      if (lev[u] < sep) A.push_back(u);
      else if (lev[u] > sep) B.push_back(u);
      else S.push_back(u);
    }
    for (int u : ord) lev[u] = -1;
    return true;
  }

  // Minimum vertex cover of the cut's bipartite graph (side-1 boundary nodes
  // x side-2 boundary nodes, the cut edges), by augmenting paths and König's
  // construction: the smallest vertex separator that removes every cut edge
  // while keeping the remaining nodes on their sides.  On the co-visibility
  // graph (edges span up to ~3 tag spacings) it is often well below either
  // one-sided boundary.  cover[u] = 1 for the chosen nodes of comp.
  // (loc: scratch of adj.size() entries for the local numbering)
  int konig_cover(const std::vector<int> &comp, const std::vector<int> &side, int tag,
                  std::vector<char> &cover, std::vector<int> &loc) {
    std::vector<int> left, right;
    for (int u : comp) {
      bool bd = false;
      for (int v : adj[u])
        if (mark[v] == tag && side[v] != side[u]) { bd = true; break; }
      if (bd) (side[u] == 1 ? left : right).push_back(u);
    }
    std::vector<int> idx(0);
    // local numbering: left 0..nl-1, right nl..
    const int nl = (int)left.size(), nr = (int)right.size();
    for (int i = 0; i < nl; ++i) loc[left[i]] = i;
    for (int i = 0; i < nr; ++i) loc[right[i]] = nl + i;
    std::vector<std::vector<int>> g(nl);
    for (int i = 0; i < nl; ++i)
      for (int v : adj[left[i]])
        if (mark[v] == tag && side[v] == 2) g[i].push_back(loc[v] - nl);
    std::vector<int> mate_l(nl, -1), mate_r(nr, -1), seen(nr, -1);
    // Kuhn's augmenting paths (iterative DFS), greedy initial matching
    for (int i = 0; i < nl; ++i)
      for (int r : g[i])
        if (mate_r[r] < 0) { mate_l[i] = r; mate_r[r] = i; break; }
    std::vector<std::pair<int, int>> st;
    std::vector<int> par_r(nr, -1);
    for (int i0 = 0; i0 < nl; ++i0) {
      if (mate_l[i0] >= 0) continue;
      st.assign(1, {i0, 0});
      int found = -1;
      while (!st.empty() && found < 0) {
        auto &[i, k] = st.back();
        if (k >= (int)g[i].size()) { st.pop_back(); continue; }
        const int r = g[i][k++];
        if (seen[r] == i0) continue;
        seen[r] = i0;
        par_r[r] = i;
        if (mate_r[r] < 0) found = r;
        else st.push_back({mate_r[r], 0});
      }
      for (int r = found; r >= 0;) {   // flip the path
        const int i = par_r[r], nxt = mate_l[i];
        mate_l[i] = r;
        mate_r[r] = i;
        r = nxt;
      }
    }
    // König: Z = reachable from unmatched left nodes by alternating paths
    std::vector<char> zl(nl, 0), zr(nr, 0);
    std::vector<int> q;
    for (int i = 0; i < nl; ++i)
      if (mate_l[i] < 0) { zl[i] = 1; q.push_back(i); }
    for (size_t h = 0; h < q.size(); ++h)
      for (int r : g[q[h]])
        if (!zr[r] && mate_l[q[h]] != r) {
          zr[r] = 1;
          const int i = mate_r[r];
          if (i >= 0 && !zl[i]) { zl[i] = 1; q.push_back(i); }
        }
    int n = 0;
    for (int i = 0; i < nl; ++i) if (!zl[i]) { cover[left[i]] = 1; ++n; }
    for (int r = 0; r < nr; ++r) if (zr[r]) { cover[right[r]] = 1; ++n; }
    (void)idx;
    return n;
  }

  // Geometric separator: cut the component by a plane normal to one of its
  // principal axes at a quantile of the projections; the separator is the
  // minimum vertex cover of the cut edges (konig_cover).  The best
  // (smallest, then most balanced) of several cuts is kept.
  bool geometric_separator(std::vector<int> &comp, int tag, std::vector<int> &A, std::vector<int> &B,
                           std::vector<int> &S) {
    const int m = (int)comp.size();
    double c[3] = {0, 0, 0}, C[9] = {0};
    for (int u : comp)
      for (int a = 0; a < 3; ++a) c[a] += xyz[3L * u + a] / m;
    for (int u : comp)
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[3 * a + b] += (xyz[3L * u + a] - c[a]) * (xyz[3L * u + b] - c[b]);
    // two leading principal axes by power iteration with deflation
    double axes[2][3];
    double D[9];
    std::copy(C, C + 9, D);
    for (int k = 0; k < 2; ++k) {
      double v[3] = {1.0, 0.7, 0.3};
      double lam = 0.0;
      for (int it = 0; it < 100; ++it) {
        double w[3];
        for (int a = 0; a < 3; ++a) w[a] = D[3 * a] * v[0] + D[3 * a + 1] * v[1] + D[3 * a + 2] * v[2];
        const double nw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (nw == 0.0) break;
        for (int a = 0; a < 3; ++a) v[a] = w[a] / nw;
        lam = nw;
      }
      for (int a = 0; a < 3; ++a) axes[k][a] = v[a];
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) D[3 * a + b] -= lam * v[a] * v[b];
    }
    // (fast, components of up to 512 tags: half the directions and every
    // other quantile, a quarter of the König covers -- the order was most of
    // an incremental reload; a slightly larger fill, e.g. cfg2 213 tiles
    // against 205)
    const bool big = !fast || m > 512;
    const int n_dir = big ? 6 : 3, n_q = 20, q_step = big ? 1 : 2;
    // each direction's best cut (its own scratch; large components search the
    // directions concurrently), then the first best over the directions in
    // order: the serial search's choice
    std::vector<double> dir_score(n_dir, -1.0);
    std::vector<std::vector<int>> dir_side(n_dir);
    auto search = [&](int k) {
      std::vector<int> side(adj.size(), 0), loc(adj.size(), -1);
      std::vector<char> cover(adj.size(), 0);
      std::vector<std::pair<double, int>> pr(m);
      double &best_score = dir_score[k];
      std::vector<int> &best_side = dir_side[k];
      // cut directions in the plane of the two principal axes
      const double ang = M_PI * k / n_dir, ca = std::cos(ang), sa = std::sin(ang);
      double dir[3];
      for (int a = 0; a < 3; ++a) dir[a] = ca * axes[0][a] + sa * axes[1][a];
      for (int i = 0; i < m; ++i) {
        const int u = comp[i];
        pr[i] = {dir[0] * xyz[3L * u] + dir[1] * xyz[3L * u + 1] + dir[2] * xyz[3L * u + 2], u};
      }
      std::sort(pr.begin(), pr.end());
      const int q0 = (int)std::lround(nd_qlo() * n_q);
      for (int qi = q0; qi <= n_q - q0; qi += q_step) {   // cut at quantiles 0.30 .. 0.70
        const int cut = m * qi / n_q;
        if (cut < 1 || cut >= m) continue;
        for (int i = 0; i < m; ++i) side[pr[i].second] = i < cut ? 1 : 2;
        for (int u : comp) cover[u] = 0;
        const int ssz = konig_cover(comp, side, tag, cover, loc);
        int na = 0, nbb = 0;
        for (int u : comp)
          if (!cover[u]) (side[u] == 1 ? na : nbb)++;
        if (std::min(na, nbb) < (int)(nd_min_side() * m)) continue;
        // elimination-tree height in tile columns: the separator's tiles plus
        // the larger child's height, which grows about as sqrt(size) on these
        // planar graphs (cfg3's tree: ~1 tile column per sqrt(tag))
        const double score = height_score(ssz, na, nbb);
        if (best_score < 0 || score < best_score) {
          best_score = score;
          best_side.assign(m, 0);
          for (int i = 0; i < m; ++i) best_side[i] = cover[comp[i]] ? 0 : side[comp[i]];
        }
      }
    };
    if (m >= 256) host_parallel_for(n_dir, search);
    else for (int k = 0; k < n_dir; ++k) search(k);
    double best_score = -1;
    int best_k = -1;
    for (int k = 0; k < n_dir; ++k)
      if (dir_score[k] >= 0 && (best_score < 0 || dir_score[k] < best_score)) {
        best_score = dir_score[k];
        best_k = k;
      }
    if (best_score < 0) return false;
    const std::vector<int> &best_side = dir_side[best_k];
    for (int i = 0; i < m; ++i) (best_side[i] == 1 ? A : best_side[i] == 2 ? B : S).push_back(comp[i]);
    return true;
  }

  void dissect(std::vector<int> &comp, int tag, std::vector<std::vector<int>> &parts) {
    if ((int)comp.size() <= leaf) {
      leaf_part(comp, tag, parts);
      return;
    }
    std::vector<int> A, B, S;
    bool ok = false;
    if (!xyz.empty()) {
      ok = geometric_separator(comp, tag, A, B, S);
      std::vector<int> A2, B2, S2;
      if (level_separator(comp, tag, A2, B2, S2) &&
          (!ok || height_score((long)S2.size(), (long)A2.size(), (long)B2.size()) <
                      height_score((long)S.size(), (long)A.size(), (long)B.size()))) {
        A.swap(A2); B.swap(B2); S.swap(S2);
        ok = true;
      }
    } else {
      ok = level_separator(comp, tag, A, B, S);
    }
    if (!ok) {
      leaf_part(comp, tag, parts);
      return;
    }
    absorb(A, B, S, tag);
    static const bool dbg = std::getenv("ARSLAM_ND_DEBUG") != nullptr;   // debug: the dissection tree
    if (dbg) std::fprintf(stderr, "nd: comp %zu -> A %zu B %zu S %zu\n", comp.size(), A.size(), B.size(), S.size());
    const int ta = ++next_tag, tb = ++next_tag, ts = ++next_tag;
    for (int u : A) mark[u] = ta;
    for (int u : B) mark[u] = tb;
    for (int u : S) mark[u] = ts;
    std::vector<std::vector<int>> pb;
    host_fork2(std::min(A.size(), B.size()) >= 128, [&] { run(A, ta, parts); }, [&] { run(B, tb, pb); });
    for (auto &q : pb) parts.push_back(std::move(q));
    parts.push_back(S);
  }

  // Grow the separator into the larger side (nodes adjacent to it first) until
  // its 6 rows per tag fill whole 64-row tiles: rows that would otherwise be
  // alignment padding become separator rows, and the children shrink.  Any
  // superset of a separator taken from one side still separates.
  void absorb(std::vector<int> &A, std::vector<int> &B, std::vector<int> &S, int tag) {
    const long rows = 6L * (long)S.size();
    int extra = (int)((round_up(rows, kTileRows) - rows) / 6);
    std::vector<int> &X = A.size() >= B.size() ? A : B;
    if (extra <= 0 || (int)X.size() <= extra) return;
    const int tx = ++next_tag;
    for (int u : X) mark[u] = tx;
    std::vector<char> take(adj.size(), 0);
    std::vector<int> frontier;
    for (int u : S)
      for (int v : adj[u])
        if (mark[v] == tx && !take[v] && extra > 0) { take[v] = 1; frontier.push_back(v); --extra; }
    for (size_t h = 0; h < frontier.size() && extra > 0; ++h)
      for (int v : adj[frontier[h]])
        if (mark[v] == tx && !take[v] && extra > 0) { take[v] = 1; frontier.push_back(v); --extra; }
    std::vector<int> keep;
    for (int u : X) (take[u] ? S : keep).push_back(u);
    for (int u : X) mark[u] = tag;
    X.swap(keep);
  }

  void leaf_part(std::vector<int> &comp, int tag, std::vector<std::vector<int>> &parts) {
    // within a leaf keep BFS order (locality)
    std::vector<int> ord = bfs(comp[0], adj, mark, tag, lev);
    for (int u : ord) lev[u] = -1;
    parts.push_back(ord);
  }
};

}  // namespace

std::vector<int> rcm_order(int n, const std::vector<std::vector<int>> &adj) {
  std::vector<int> order;
  order.reserve(n);
  std::vector<int> mark(n, 0), lev(n, -1);
  std::vector<char> done(n, 0);
  for (;;) {
    int start = -1;
    for (int v = 0; v < n; ++v)
      if (!done[v] && (start < 0 || adj[v].size() < adj[start].size())) start = v;
    if (start < 0) break;
    start = peripheral(start, adj, mark, 0, lev);
    std::deque<int> q{start};
    done[start] = 1;
    while (!q.empty()) {
      const int u = q.front();
      q.pop_front();
      order.push_back(u);
      std::vector<int> nb;
      for (int v : adj[u])
        if (!done[v]) { done[v] = 1; nb.push_back(v); }
      std::stable_sort(nb.begin(), nb.end(),
                       [&](int a, int b) { return adj[a].size() < adj[b].size(); });
      for (int v : nb) q.push_back(v);
    }
  }
  std::reverse(order.begin(), order.end());
  return order;
}

std::vector<std::vector<int>> nd_parts(int n, const std::vector<std::vector<int>> &adj, int leaf,
                                       const std::vector<double> &xyz, bool fast) {
  Dissector d(adj, xyz, leaf);
  d.fast = fast;
  std::vector<int> all(n);
  for (int i = 0; i < n; ++i) all[i] = i;
  std::vector<std::vector<int>> parts;
  d.run(all, 0, parts);
  return parts;
}

}  // namespace arslam
