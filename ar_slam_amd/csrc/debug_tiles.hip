// debug_tiles.hip -- component entry points (include/arslam_lm_debug.h) over the
// tile Cholesky and what is built on its factor: a dense n x n matrix on a
// lower tile pattern goes through the plan, the executors, the selected
// inverse or the multi-right-hand-side solve alone, and comes back dense.
// One fixture owns the pattern, the plans, the packing and the buffers; each
// entry point checks its arguments, builds the fixture, launches its kernels
// and unpacks.
#include "hip_host.h"
#include "llt_plan.h"
#include "lm_cov.h"
#include "lm_problem.h"
#include "arslam_lm.h"
#include "arslam_lm_debug.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
using namespace arslam;

// The lower tile pattern a component entry factors: the given one (null = dense) plus what is
// always taken, the diagonal tiles and, with last_row, the last tile row (it holds the right-hand side).
std::vector<uint8_t> taken_pattern(int T, const unsigned char *given, bool last_row) {
  std::vector<uint8_t> p((size_t)T * T, 0);
  for (int i = 0; i < T; ++i)
    for (int j = 0; j <= i; ++j)
      p[(size_t)i * T + j] = i == j || (last_row && i == T - 1) || !given || given[(size_t)i * T + j];
  return p;
}

// Column classes of a two-phase plan on one rank (null = one phase): 0 / 1 only, and the class-1
// columns closed under the elimination tree's parent (phase 0 runs first, so a class-1 column
// under a class-0 ancestor would update a column already factored).
bool tile_classes(int T, const std::vector<uint8_t> &taken, const unsigned char *col_class, std::vector<int> &cls) {
  cls.clear();
  if (!col_class) return true;
  std::vector<uint8_t> filled = taken;
  std::vector<int> parent;
  tile_fill(T, filled, parent);
  cls.assign(col_class, col_class + T);
  for (int k = 0; k < T; ++k)
    if (cls[k] > 1 || (cls[k] == 1 && parent[k] >= 0 && cls[parent[k]] != 1)) return false;
  return true;
}

void tile_plan_facts(const LltPlan &plan, arslam_tile_plan_facts *f) {
  std::memset(f, 0, sizeof(*f));
  f->tiles_per_side = plan.T;
  f->n_assembled = plan.n_assembled;
  f->n_tiles = plan.n_tiles;
  f->n_levels = plan.nlev;
  f->n_split = (long)plan.h_split.size();
  f->n_dag_tasks = plan.n_dag_tasks;
  f->fill_first_ok = plan.fill_first_ok ? 1 : 0;
  f->phase_split = plan.n_phases > 1 ? plan.phase_split : plan.n_dag_tasks;
  for (int c : plan.h_dag_cont) f->n_cont_tasks += c >= 0;
}

// the k_factor_dag grids a request of n_workgroups gives the plan's launch (one phase) or launches
void tile_plan_grids(const LltPlan &plan, int n_workgroups, int grid[2]) {
  const long n0 = plan.n_phases > 1 ? plan.phase_split : plan.n_dag_tasks, n1 = plan.n_dag_tasks - n0;
  grid[0] = n0 > 0 ? dag_launch_grid(n0, n_workgroups) : 0;
  grid[1] = n1 > 0 ? dag_launch_grid(n1, n_workgroups) : 0;
}

// the workgroups asked of the persistent executor: ARSLAM_DAG_GRID or 512, at most the
// resident workgroups (the claim cap is half the grid)
int dag_grid_request() {
  const char *eg = std::getenv("ARSLAM_DAG_GRID");
  int grid = eg ? std::max(1, std::atoi(eg)) : 512;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
    grid = std::min(grid, kDagWorkgroupsPerCu * cus);
  return grid;
}

// A dense n x n matrix as the tile Cholesky sees a reduced system: N = n + 1 rows rounded up to
// whole tiles, the right-hand side as row n.  Owns the plans and every device buffer.
struct TileFixture {
  const long n, N;
  const int T;
  std::vector<uint8_t> pattern;   // the tiles taken; build() fills it in to the factor's
  std::vector<uint8_t> given;     // the tiles taken, kept by build(): the ones pack() writes
  std::vector<int> cls;
  LltPlan plan;
  SelinvPlan sp;
  TileSolvePlan tp;
  std::vector<double> tiles;   // the host image of S, then of what fetch_tiles() brought back
  DevBuf<double> S, Z, panels, z, y;
  DevBuf<int> flag;

  TileFixture(long n_, const unsigned char *tile_pattern, bool last_row)
      : n(n_), N((n_ + 1 + kTile - 1) / kTile * kTile), T((int)(N / kTile)),
        pattern(taken_pattern(T, tile_pattern, last_row)) {}
  TileFixture(const TileFixture &) = delete;
  TileFixture &operator=(const TileFixture &) = delete;
  ~TileFixture() {
    selinv_plan_free(sp);
    tile_solve_plan_free(tp);
    llt_plan_free(plan);
  }

  bool classes(const unsigned char *col_class) { return tile_classes(T, pattern, col_class, cls); }

  void build() {
    given = pattern;
    llt_plan_build(plan, T, N, pattern, 0, cls.empty() ? nullptr : &cls);   // (pattern: filled in place)
    tiles.assign((size_t)plan.n_tiles * 4096, 0.0);
    flag.alloc(1);
    HIP_CHECK(hipMemset(flag.p, 0, sizeof(int)));
  }

  // S on the device: the lower matrix on the given tiles, b (null: zero) as row n with the
  // pivot 1e300, identity padding; the fill tiles zero, or quiet NaNs where the fill-first
  // store has to write them first
  void pack(const double *A, const double *b, bool nan_fill) {
    if (nan_fill) std::fill(tiles.begin() + (size_t)plan.n_assembled * 4096, tiles.end(), std::nan(""));
    for (int ti = 0; ti < T; ++ti)
      for (int tj = 0; tj <= ti; ++tj) {
        if (!given[(size_t)ti * T + tj]) continue;
        double *t = tiles.data() + (size_t)plan.h_tile_id[(size_t)ti * T + tj] * 4096;
        for (int r = 0; r < 64; ++r)
          for (int c = 0; c < 64; ++c) {
            const long i = ti * 64L + r, j = tj * 64L + c;
            t[r * 64 + c] = j > i ? 0.0 : i < n ? A[i * n + j] : i == n ? (j == n ? 1e300 : b ? b[j] : 0.0) : i == j ? 1.0 : 0.0;
          }
      }
    S.alloc(tiles.size());
    HIP_CHECK(hipMemcpy(S.p, tiles.data(), tiles.size() * sizeof(double), hipMemcpyHostToDevice));
  }

  // after the launches: wait for them and fetch the flag
  void finish(int *info) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(info, flag.p, sizeof(int), hipMemcpyDeviceToHost));
  }
  void fetch_tiles(const DevBuf<double> &src) {   // S or Z into the host image
    HIP_CHECK(hipMemcpy(tiles.data(), src.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost));
  }

  void unpack_lower(double *L_out) const {
    for (long i = 0; i < n; ++i)
      for (long j = 0; j < n; ++j) {
        const int id = j <= i ? plan.h_tile_id[(size_t)(i / 64) * T + j / 64] : -1;
        L_out[i * n + j] = id < 0 ? 0.0 : tiles[(size_t)id * 4096 + (i % 64) * 64 + (j % 64)];
      }
  }

  void unpack_symmetric(double *Z_out) const {
    for (long i = 0; i < n; ++i)
      for (long j = 0; j < n; ++j) {
        // tile (ti, tj), ti >= tj, holds Z's rows of ti; the upper triangle is its mirror
        const long ti = std::max(i, j) / 64, tj = std::min(i, j) / 64;
        const int id = plan.h_tile_id[(size_t)ti * T + tj];
        const long r = ti == tj ? i % 64 : std::max(i, j) % 64, c = ti == tj ? j % 64 : std::min(i, j) % 64;
        Z_out[i * n + j] = id < 0 ? 0.0 : tiles[(size_t)id * 4096 + r * 64 + c];
      }
  }
};
}  // namespace

extern "C" int arslam_debug_tile_plan(int T, const unsigned char *tile_pattern, const unsigned char *col_class,
                                      unsigned char *pattern_out, arslam_tile_plan_facts *facts) {
  if (T <= 0 || !facts) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    std::vector<uint8_t> pattern = taken_pattern(T, tile_pattern, true);
    std::vector<int> cls;
    api_check(tile_classes(T, pattern, col_class, cls), ARSLAM_E_INVALID_ARG, "col_class: not 0 / 1, or not closed");
    LltPlan plan;
    llt_plan_symbolic(plan, T, (long)T * kTile, pattern, col_class ? &cls : nullptr);
    if (pattern_out) std::memcpy(pattern_out, pattern.data(), pattern.size());
    tile_plan_facts(plan, facts);
    tile_plan_grids(plan, 512, facts->grid);   // (the default request; no device to clamp it by)
    facts->dag_valid = dag_check(plan) ? 1 : 0;
    if (facts->dag_valid) facts->dag_valid = dag_simulate_all(plan);
  });
}

extern "C" int arslam_debug_dense_llt(long n, double *A, const double *b, double *y, int *info) {
  return arslam_debug_dense_llt_ex(n, A, b, y, info, 0);
}

extern "C" int arslam_debug_dense_llt_ex(long n, double *A, const double *b, double *y, int *info,
                                         int executor) {
  // (in place: arslam_debug_tile_llt has read all of A before it writes L)
  return arslam_debug_tile_llt(n, A, b, nullptr, executor == 1 ? 1 : 0, nullptr, 0, A, y, nullptr, info, nullptr);
}

extern "C" int arslam_debug_tile_llt(long n, const double *A, const double *b, const unsigned char *tile_pattern,
                                     int executor, const unsigned char *col_class, unsigned flags, double *L_out,
                                     double *y, unsigned char *pattern_out, int *info,
                                     arslam_tile_plan_facts *facts) {
  if (n <= 0 || !A || !b || !L_out || !y || !info || executor < 0 || executor > 1 || (flags & ~1u))
    return ARSLAM_E_INVALID_ARG;
  const bool fill_first = (flags & 1u) != 0, two_phase = col_class != nullptr;
  if ((fill_first || two_phase) && executor != 1) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    TileFixture fx(n, tile_pattern, true);
    api_check(fx.classes(col_class), ARSLAM_E_INVALID_ARG, "col_class: not 0 / 1, or not closed");
    fx.build();
    api_check(!fill_first || fx.plan.fill_first_ok, ARSLAM_E_INVALID_ARG, "the plan has no fill-first store");
    if (pattern_out) std::memcpy(pattern_out, fx.pattern.data(), fx.pattern.size());
    fx.pack(A, b, fill_first);
    fx.z.alloc(fx.N);
    fx.y.alloc(fx.N);
    const int grid = dag_grid_request();
    if (facts) {
      tile_plan_facts(fx.plan, facts);
      if (executor == 1) tile_plan_grids(fx.plan, grid, facts->grid);
    }
    double *S = fx.S.p;
    int *flag = fx.flag.p;
    if (executor == 1 && two_phase) {
      // as factor_reduced launches them: one reset, phase 0, (one rank: no exchange,) phase 1
      launch_exec_reset(fx.plan, flag, 0);
      launch_dense_llt_dag(fx.plan, S, flag, 0, grid, nullptr, nullptr, false, 0);
      launch_dense_llt_dag(fx.plan, S, flag, 0, grid, nullptr, nullptr, false, 1);
    } else if (executor == 1) {
      launch_dense_llt_dag(fx.plan, S, flag, 0, grid, nullptr, nullptr, true, -1,
                           fill_first ? fx.plan.n_assembled : LONG_MAX);
    } else {
      launch_dense_llt(fx.plan, S, flag, 0);
    }
    if (executor == 1) launch_dense_back_solve_dag(fx.plan, S, n, fx.y.p, flag, 0, grid);
    else launch_dense_back_solve(fx.plan, S, n, fx.z.p, fx.y.p, flag, 0);
    launch_scatter_diag(fx.plan, S, 0);
    fx.finish(info);
    fx.fetch_tiles(fx.S);
    HIP_CHECK(hipMemcpy(y, fx.y.p, n * sizeof(double), hipMemcpyDeviceToHost));
    fx.unpack_lower(L_out);
  });
}

extern "C" int arslam_debug_selinv(long n, const double *A, const unsigned char *tile_pattern, double *Z_out,
                                   unsigned char *pattern_out, int *info) {
  if (n <= 0 || !A || !Z_out || !info) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    TileFixture fx(n, tile_pattern, false);
    fx.build();
    selinv_plan_build(fx.plan, fx.sp, 0);
    if (pattern_out) std::memcpy(pattern_out, fx.pattern.data(), fx.pattern.size());
    fx.pack(A, nullptr, false);
    fx.Z.alloc(fx.tiles.size());
    HIP_CHECK(hipMemset(fx.Z.p, 0, fx.tiles.size() * sizeof(double)));
    launch_dense_llt(fx.plan, fx.S.p, fx.flag.p, 0);
    launch_selinv(fx.plan, fx.sp, fx.S.p, n, fx.Z.p, fx.flag.p, 0);
    fx.finish(info);
    fx.fetch_tiles(fx.Z);
    fx.unpack_symmetric(Z_out);
  });
}

extern "C" int arslam_debug_tile_solve(long n, const double *A, const unsigned char *tile_pattern, int nrhs,
                                       const double *B, double *X_out, int *info) {
  if (n <= 0 || nrhs <= 0 || !A || !B || !X_out || !info) return ARSLAM_E_INVALID_ARG;
  return api_guarded([&] {
    TileFixture fx(n, tile_pattern, false);
    fx.build();
    tile_solve_plan_build(fx.plan, fx.tp, 0);
    fx.pack(A, nullptr, false);
    // the right-hand sides, sixty columns to a panel of T row-major 64x64 tiles
    const int T = fx.T, per_panel = 6 * kCovPanelBlocks;
    const int n_panels = (nrhs + per_panel - 1) / per_panel;
    std::vector<double> panels((size_t)n_panels * T * 4096, 0.0);
    const auto pel = [&](long r, int c) -> double & {
      return panels[((size_t)(c / per_panel) * T + r / 64) * 4096 + (r % 64) * 64 + c % per_panel];
    };
    for (long r = 0; r < n; ++r)
      for (int c = 0; c < nrhs; ++c) pel(r, c) = B[r * nrhs + c];
    fx.panels.alloc(panels.size());
    HIP_CHECK(hipMemcpy(fx.panels.p, panels.data(), panels.size() * sizeof(double), hipMemcpyHostToDevice));
    launch_dense_llt(fx.plan, fx.S.p, fx.flag.p, 0);
    launch_tile_solve(fx.plan, fx.tp, fx.S.p, n, fx.panels.p, n_panels, nullptr, nullptr, fx.flag.p, 0);
    fx.finish(info);
    HIP_CHECK(hipMemcpy(panels.data(), fx.panels.p, panels.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (long r = 0; r < n; ++r)
      for (int c = 0; c < nrhs; ++c) X_out[r * nrhs + c] = pel(r, c);
  });
}
