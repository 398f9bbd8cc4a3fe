// cov_pairs.hip -- cross-covariance blocks between any two parameter blocks
// (arslam_lm_covariance_pairs): a triangular solve of the reduced system's tile
// factor with many right-hand sides, and the two small kernels around it.
//
// The selected inverse (selinv.hip) holds Z = S^{-1} on the factor's filled
// tile pattern only, so the block of two tags far apart under nested
// dissection is not in it.  Here whole columns of Z are solved for instead:
//   X = L^{-T} L^{-1} B
// with B one 6-column block per distinct right-hand parameter block, ten of
// them (and four zero columns) to a 64-column panel stored as T tiles of 64x64:
//   forward   Y_k = L_kk^{-1} (B_k - sum_{j<k, (k,j) in pattern} L_kj Y_j)   leaves first
//   backward  X_k = L_kk^{-T} (Y_k - sum_{j in I_k} L_jk^T X_j)              root level first
// in place in the panel.  The levels are the elimination tree's heights (the
// backward solve's, LltPlan::h_bs_off): the columns j a forward step reads are
// its descendants, those a backward step reads its ancestors.  One workgroup
// per (tile column, panel), the j-sum serial inside it in plan order, plain
// grid launches per level: no tickets, no waits between workgroups, no
// atomics, bitwise reproducible.
//
// A right-hand block is non-zero only in the tile rows of its reduced rows, and
// a pair reads X only in the tile rows of its other block.  Per panel the host
// passes two byte masks over the tile rows, each closed under the elimination
// tree's ancestors: `active` (where B, hence Y, can be non-zero: the forward
// pass skips the other tile rows and every product with an inactive Y_j, all
// exactly zero, so no bit changes) and `needed` (the rows of X somebody reads:
// the backward pass computes those alone; a column reads its ancestors only).
//
// The solves read the factor itself: S after launch_dense_llt /
// launch_dense_llt_dag, before (or without) launch_selinv, whose k_selinv_g
// overwrites the off-diagonal tiles with L_jk X_kk in place.
//
// Masking as in the selected inverse: row nR is the right-hand side the LM step
// folds into the factor (pivot 1e300) and the rows after it identity padding;
// rows >= nR of every factor tile and rows and columns >= nR of L_kk^{-1} are
// read as zero, so those rows contribute exactly nothing and stay zero in X.
#include "cov_device.h"

#include <algorithm>
#include <stdexcept>

namespace arslam {

namespace {

// 256-thread load of a 64x64 row-major tile into LDS (pitch LQ): element
// (r, c) to lds[r][c], or to lds[c][r] (tr); rows >= rlim and columns >= clim
// of the tile read as 0
__device__ __forceinline__ void load_tile_rc(const double *__restrict__ g, double *lds, int tid, bool tr, int rlim,
                                             int clim) {
  dbl2 v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    v[q] = *reinterpret_cast<const dbl2 *>(g + r * T64 + c2);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    const double x = (r < rlim && c2 < clim) ? v[q].x : 0.0;
    const double y = (r < rlim && c2 + 1 < clim) ? v[q].y : 0.0;
    if (tr) {
      lds[c2 * LQ + r] = x;
      lds[(c2 + 1) * LQ + r] = y;
    } else {
      *reinterpret_cast<dbl2 *>(lds + r * LQ + c2) = dbl2{x, y};
    }
  }
}

// valid rows of tile row i: those below the rhs row nR
__device__ __forceinline__ int tile_lim(int i, long nR) {
  const long l = nR - (long)i * T64;
  return l >= T64 ? T64 : l > 0 ? (int)l : 0;
}

// The tail of both passes: the panel tile Pk minus the accumulated sum goes to
// sB transposed (sB[c][r] = (Pk - acc)[r][c]), the masked diagonal inverse to
// sA (transposed for the backward pass), and their product back to Pk.
__device__ __forceinline__ void apply_diag_inverse(double *__restrict__ Pk, const double *__restrict__ Xkk, bool tr,
                                                   int lim, double *sA, double *sB, int tid, const dbl4 acc[4]) {
  __syncthreads();   // the last product's fragments consumed
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int row, col;
      acc_pos(tid, q, reg, row, col);
      sB[col * LQ + row] = Pk[row * T64 + col] - acc[q][reg];
    }
  load_tile_rc(Xkk, sA, tid, tr, lim, lim);
  __syncthreads();
  dbl4 out[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  gemm64_nt(sA, sB, tid, out);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int row, col;
      acc_pos(tid, q, reg, row, col);
      Pk[row * T64 + col] = out[q][reg];
    }
}

// Forward step of one level: workgroup (x, y) takes column cols[b0 + x] of
// panel y.  flist[fbeg[b] .. fbeg[b + 1]): the off-diagonal tiles (k, j) of
// tile row k = cols[b], ascending j, as {j, tile id}.
__global__ __launch_bounds__(256) void k_tsolve_fwd(const double *__restrict__ S, const double *__restrict__ Xinv,
                                                    long nR, double *__restrict__ B, int T,
                                                    const int *__restrict__ cols, const int *__restrict__ fbeg,
                                                    const int2 *__restrict__ flist, int b0,
                                                    const unsigned char *__restrict__ active,
                                                    const int *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) double sA[T64 * LQ];
  __shared__ __attribute__((aligned(16))) double sB[T64 * LQ];
  if (*flag) return;
  const int tid = threadIdx.x;
  const int b = b0 + blockIdx.x, k = cols[b];
  const unsigned char *act = active ? active + (long)blockIdx.y * T : nullptr;
  if (act && !act[k]) return;   // B_k and every Y_j of its row are zero: so is Y_k, as the panel already says
  double *Bp = B + (long)blockIdx.y * T * (T64 * T64);
  const int lim = tile_lim(k, nR);
  dbl4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  bool first = true;
  for (int q = fbeg[b]; q < fbeg[b + 1]; ++q) {
    const int2 t = flist[q];
    if (act && !act[t.x]) continue;     // Y_j = 0
    if (!first) __syncthreads();        // the previous product's fragments consumed
    first = false;
    load_tile_rc(S + (long)t.y * (T64 * T64), sA, tid, false, lim, T64);       // L_kj, its rows >= nR zero
    load_tile_rc(Bp + (long)t.x * (T64 * T64), sB, tid, true, T64, T64);       // sB[c][r] = Y_j[r][c]
    __syncthreads();
    gemm64_nt(sA, sB, tid, acc);
  }
  apply_diag_inverse(Bp + (long)k * (T64 * T64), Xinv + (long)k * (T64 * T64), false, lim, sA, sB, tid, acc);
}

// Backward step of one level: the backward solve's lists (LltPlan::bs_cols,
// bs_gather, bs_gbeg, bs_gtile), column cols[b0 + x] of panel y.
__global__ __launch_bounds__(256) void k_tsolve_bwd(const double *__restrict__ S, const double *__restrict__ Xinv,
                                                    long nR, double *__restrict__ B, int T,
                                                    const int *__restrict__ cols, const int *__restrict__ gbeg,
                                                    const int2 *__restrict__ gather, const int *__restrict__ gtile,
                                                    int b0, const unsigned char *__restrict__ needed,
                                                    const int *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) double sA[T64 * LQ];
  __shared__ __attribute__((aligned(16))) double sB[T64 * LQ];
  if (*flag) return;
  const int tid = threadIdx.x;
  const int b = b0 + blockIdx.x, k = cols[b];
  if (needed && !needed[(long)blockIdx.y * T + k]) return;   // nobody reads X_k (its ancestors are all needed)
  double *Bp = B + (long)blockIdx.y * T * (T64 * T64);
  dbl4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int q = gbeg[b]; q < gbeg[b + 1]; ++q) {
    const int j = gather[q].x;
    if (q > gbeg[b]) __syncthreads();
    load_tile_rc(S + (long)gtile[q] * (T64 * T64), sA, tid, true, tile_lim(j, nR), T64);   // sA[r][a] = L_jk[a][r]
    load_tile_rc(Bp + (long)j * (T64 * T64), sB, tid, true, T64, T64);                     // sB[c][a] = X_j[a][c]
    __syncthreads();
    gemm64_nt(sA, sB, tid, acc);
  }
  apply_diag_inverse(Bp + (long)k * (T64 * T64), Xinv + (long)k * (T64 * T64), true, tile_lim(k, nR), sA, sB, tid,
                     acc);
}

// ---------------------------------------------------------------------------
// Right-hand sides and blocks (arslam_lm_covariance_pairs).  A block of the
// device problem is {role, index}: kCovFocal, kCovF (f-block = reduced side),
// kCovE (e-block = eliminated side).

// One wavefront per distinct right-hand block, into its 6 columns of the
// (zeroed) panels: unit columns at the reduced rows of the focal (one column)
// or an f-block; -Y^T = -(R^{-1} G)^T scattered to the local columns' reduced
// rows for an e-block (nothing when its R is singular: k_cov_pair_blocks
// reports that).
__global__ __launch_bounds__(kWave) void k_cov_pair_rhs(DevProblem P, const double *__restrict__ Gb,
                                                        const double *__restrict__ Rb, const int2 *__restrict__ rhs,
                                                        double *__restrict__ B, int T) {
  __shared__ double Ri[36];
  __shared__ int ok;
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int2 blk = rhs[slot];
  if (blk.x == kCovFocal) {
    if (lane == 0 && P.cam_row >= 0) *panel_elem(B, T, slot, P.cam_row, 0) = 1.0;
    return;
  }
  if (blk.x == kCovF) {
    const int row = P.tag_row[blk.y];
    if (lane < 6 && row >= 0) *panel_elem(B, T, slot, row + lane, lane) = 1.0;
    return;
  }
  const int c = blk.y;
  if (lane == 0) ok = r_inverse(Rb + 36L * c, Ri) ? 1 : 0;
  __syncthreads();
  if (!ok) return;
  const int b0 = P.cap_blk_start[c], m = 1 + 6 * (P.cap_blk_start[c + 1] - b0);
  const double *G = Gb + 6L * (c + 6L * b0);
  for (int p = lane; p < m; p += kWave) {
    const long row = local_col_row(P, b0, p);
    if (row < 0) continue;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double y = 0.0;
#pragma unroll
      for (int q = a; q < 6; ++q) y += Ri[6 * a + q] * G[6 * p + q];
      *panel_elem(B, T, slot, row, a) = -y;
    }
  }
}

// One wavefront per unordered pair (a, b), b the solved side whose columns X_b
// sit in panel slot t.slot: the scaled block, rows of a by columns of b,
//   a the focal or an f-block:  X_b[rows(a), :]
//   a an e-block:               -Y_a X_b[loc(a), :]  (+ R_a^{-1} R_a^{-T} when a = b)
// then unscaled by the two blocks' Jacobi scales.  The focal has one row (or
// column), the other five are 0.  a = b: the lower triangle, mirrored.  X may
// be null (no reduced system): only the a = b e-block term survives.
// status: 0 computed, 2 an e-block's R is singular (or *flag != 0): -1.
__global__ __launch_bounds__(kWave) void k_cov_pair_blocks(DevProblem P, const double *__restrict__ X, int T,
                                                           const double *__restrict__ scale,
                                                           const double *__restrict__ Gb,
                                                           const double *__restrict__ Rb,
                                                           const CovPairTask *__restrict__ tasks,
                                                           double *__restrict__ outp, int *__restrict__ status,
                                                           const int *__restrict__ flag) {
  __shared__ double Ria[36], Rib[36], V[36];
  __shared__ int ok;
  const int lane = threadIdx.x;
  const CovPairTask t = tasks[blockIdx.x];
  double *out = outp + 36L * t.out;
  if (lane == 0) {
    bool good = *flag == 0;
    if (good && t.role_a == kCovE) good = r_inverse(Rb + 36L * t.idx_a, Ria);
    if (good && t.role_b == kCovE) good = r_inverse(Rb + 36L * t.idx_b, Rib);
    ok = good ? 1 : 0;
  }
  __syncthreads();
  if (!ok) {
    if (lane < 36) out[lane] = -1.0;
    if (lane == 0) status[t.out] = 2;
    return;
  }
  const bool same = t.role_a == t.role_b && t.idx_a == t.idx_b;
  const int i = lane / 6, j = lane % 6;
  const int na = t.role_a == kCovFocal ? 1 : 6, nb = t.role_b == kCovFocal ? 1 : 6;
  const double *Xs = X ? panel_elem(const_cast<double *>(X), T, t.slot, 0, 0) : nullptr;
  // X_b[r][j]
  auto xel = [&](long r) -> double { return Xs[(r >> 6) * (long)(T64 * T64) + (r & 63) * T64 + j]; };
  const auto slot0 = [&](int role, int idx) -> long {
    return role == kCovFocal ? 0L : role == kCovE ? 3 + 6L * idx : 3 + 6L * P.nc + 6L * idx;
  };
  double v = 0.0;
  if (t.role_a != kCovE) {
    const long ra = t.role_a == kCovFocal ? P.cam_row : P.tag_row[t.idx_a];
    if (lane < 36 && i < na && j < nb && Xs && ra >= 0) v = xel(ra + i);
  } else {
    const int c = t.idx_a;
    const int b0 = P.cap_blk_start[c], m = 1 + 6 * (P.cap_blk_start[c + 1] - b0);
    const double *G = Gb + 6L * (c + 6L * b0);
    if (lane < 36) {   // V = G X_b[loc(a), :], the local columns in order
      double s = 0.0;
      if (Xs && j < nb)
        for (int p = 0; p < m; ++p) {
          const long row = local_col_row(P, b0, p);
          if (row >= 0) s += G[6 * p + i] * xel(row);
        }
      V[lane] = s;
    }
    __syncthreads();
    if (lane < 36 && j < nb) {
      for (int q = i; q < 6; ++q) v -= Ria[6 * i + q] * V[6 * q + j];
      if (same) {
        double u = 0.0;
        for (int q = (i > j ? i : j); q < 6; ++q) u += Ria[6 * i + q] * Ria[6 * j + q];
        v += u;
      }
    }
  }
  if (lane < 36) {
    if (i < na && j < nb) v *= scale[slot0(t.role_a, t.idx_a) + i] * scale[slot0(t.role_b, t.idx_b) + j];
    else v = 0.0;
    if (!same) {
      out[lane] = v;
    } else if (i >= j) {
      out[6 * i + j] = v;
      out[6 * j + i] = v;
    }
  }
  if (lane == 0) status[t.out] = 0;
}

}  // namespace

void tile_solve_plan_build(const LltPlan &P, TileSolvePlan &tp, hipStream_t s) {
  tile_solve_plan_free(tp);
  if (P.n_phases != 1) throw std::runtime_error("tile solve: one-rank plans only");
  const int T = P.T;
  std::vector<int> &fbeg = tp.h_fbeg;
  std::vector<int2> &flist = tp.h_flist;
  fbeg.assign(1, 0);
  for (int k : P.h_bcols) {
    for (int j = 0; j < k; ++j) {
      const int id = P.h_tile_id[(size_t)k * T + j];
      if (id >= 0) flist.push_back(make_int2(j, id));
    }
    fbeg.push_back((int)flist.size());
  }
  tp.parent.assign(T, -1);
  for (int k = 0; k < T; ++k)
    for (int i = k + 1; i < T && tp.parent[k] < 0; ++i)
      if (P.h_tile_id[(size_t)i * T + k] >= 0) tp.parent[k] = i;
  const size_t nf = std::max<size_t>(flist.size(), 1);
  if (hipMalloc(&tp.fbeg, fbeg.size() * sizeof(int)) != hipSuccess ||
      hipMalloc(&tp.flist, nf * sizeof(int2)) != hipSuccess) {
    tile_solve_plan_free(tp);
    throw std::runtime_error("tile solve: hipMalloc");
  }
  if (hipMemcpyAsync(tp.fbeg, fbeg.data(), fbeg.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess ||
      (!flist.empty() &&
       hipMemcpyAsync(tp.flist, flist.data(), flist.size() * sizeof(int2), hipMemcpyHostToDevice, s) != hipSuccess) ||
      hipStreamSynchronize(s) != hipSuccess) {
    tile_solve_plan_free(tp);
    throw std::runtime_error("tile solve: hipMemcpy");
  }
}

void tile_solve_plan_free(TileSolvePlan &tp) {
  if (tp.fbeg) (void)hipFree(tp.fbeg);
  if (tp.flist) (void)hipFree(tp.flist);
  tp.fbeg = nullptr;
  tp.flist = nullptr;
  tp.h_fbeg.clear();
  tp.h_flist.clear();
  tp.parent.clear();
}

void tile_solve_mark(const TileSolvePlan &tp, unsigned char *mask, long row) {
  for (int k = (int)(row >> 6); k >= 0 && k < (int)tp.parent.size() && !mask[k]; k = tp.parent[k]) mask[k] = 1;
}

long tile_solve_products(const LltPlan &P, const TileSolvePlan &tp, const unsigned char *active,
                         const unsigned char *needed) {
  long n = 0;
  for (size_t b = 0; b < P.h_bcols.size(); ++b) {
    const int k = P.h_bcols[b];
    if (!active || active[k]) {
      ++n;
      for (int q = tp.h_fbeg[b]; q < tp.h_fbeg[b + 1]; ++q) n += !active || active[tp.h_flist[q].x];
    }
    if (!needed || needed[k]) n += 1 + P.h_gbeg[b + 1] - P.h_gbeg[b];
  }
  return n;
}

void launch_tile_solve(const LltPlan &P, const TileSolvePlan &tp, const double *S, long nR, double *B, int n_panels,
                       const unsigned char *active, const unsigned char *needed, const int *flag, hipStream_t s) {
  if (n_panels <= 0) return;
  const double *Xinv = P.ldiag + (long)P.T * T64 * T64;
  const int nlev = (int)P.h_bs_off.size() - 1;
  for (int l = nlev - 1; l >= 0; --l) {   // leaves first
    const int b0 = P.h_bs_off[l], nc = P.h_bs_off[l + 1] - b0;
    if (nc > 0)
      hipLaunchKernelGGL(k_tsolve_fwd, dim3((unsigned)nc, (unsigned)n_panels), dim3(256), 0, s, S, Xinv, nR, B, P.T,
                         P.bs_cols, tp.fbeg, tp.flist, b0, active, flag);
  }
  for (int l = 0; l < nlev; ++l) {   // root level first
    const int b0 = P.h_bs_off[l], nc = P.h_bs_off[l + 1] - b0;
    if (nc > 0)
      hipLaunchKernelGGL(k_tsolve_bwd, dim3((unsigned)nc, (unsigned)n_panels), dim3(256), 0, s, S, Xinv, nR, B, P.T,
                         P.bs_cols, P.bs_gbeg, P.bs_gather, P.bs_gtile, b0, needed, flag);
  }
}

void launch_cov_pair_rhs(const DevProblem &P, const double *Gb, const double *Rb, const int2 *rhs, int n_rhs,
                         double *B, hipStream_t s) {
  if (n_rhs > 0)
    hipLaunchKernelGGL(k_cov_pair_rhs, dim3((unsigned)n_rhs), dim3(kWave), 0, s, P, Gb, Rb, rhs, B, P.T);
}

void launch_cov_pair_blocks(const DevProblem &P, const double *X, const double *scale, const double *Gb,
                            const double *Rb, const CovPairTask *tasks, int n_tasks, double *out, int *status,
                            const int *flag, hipStream_t s) {
  if (n_tasks > 0)
    hipLaunchKernelGGL(k_cov_pair_blocks, dim3((unsigned)n_tasks), dim3(kWave), 0, s, P, X, P.T, scale, Gb, Rb, tasks,
                       out, status, flag);
}

}  // namespace arslam
