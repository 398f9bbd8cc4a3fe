// selinv.hip -- selected inverse Z = S^{-1} on the tile pattern of the reduced
// system's Cholesky factor (Takahashi recursion), for the marginal covariances
// of arslam_lm_covariance.
//
// After launch_dense_llt / launch_dense_llt_dag, S holds the off-diagonal
// factor tiles L_ik and LltPlan::ldiag the diagonal factors L_kk and their
// inverses X_kk.  With I_k the off-diagonal tiles of column k:
//   G_jk = L_jk X_kk                         (j in I_k; in place over L_jk)
//   Z_ik = - sum_{j in I_k} Z_ij G_jk        (i in I_k; Z_ij = Z_ji^T for i < j)
//   Z_kk = X_kk^T X_kk - sum_j G_jk^T Z_jk   (lower triangle, mirrored)
// Columns run root level first (the backward solve's levels): the Z tiles a
// column reads, (i, j) with i, j in I_k, belong to its ancestors.  Plain grid
// launches, one workgroup per tile, sums over j in plan order: no tickets, no
// waits between workgroups, no atomics, bitwise reproducible.
//
// Row nR of the matrix is the right-hand side (pivot 1e300) and the rows after
// it identity padding: rows >= nR of every G tile and rows and columns >= nR
// of X_kk are read as zero.  The leading block of a triangular inverse is the
// inverse of the leading block, so Z on the real rows is exact, and zero on
// the others.
#include "cov_device.h"

#include <algorithm>

namespace arslam {

namespace {

// 256-thread load of a 64x64 row-major tile into LDS (pitch LQ): element
// (r, c) to lds[r][c], or to lds[c][r] (tr); rows and columns >= lim read as 0
__device__ __forceinline__ void load_tile(const double *__restrict__ g, double *lds, int tid, bool tr, int lim) {
  dbl2 v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    v[q] = *reinterpret_cast<const dbl2 *>(g + r * T64 + c2);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
    const double x = (r < lim && c2 < lim) ? v[q].x : 0.0;
    const double y = (r < lim && c2 + 1 < lim) ? v[q].y : 0.0;
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

// G_jk = L_jk X_kk over every off-diagonal tile of the factor, in place
__global__ __launch_bounds__(256) void k_selinv_g(double *__restrict__ S, const int *__restrict__ tid_map, int T,
                                                  const double *__restrict__ Xinv, long nR,
                                                  const int2 *__restrict__ tasks, const int *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) double sA[T64 * LQ];
  __shared__ __attribute__((aligned(16))) double sB[T64 * LQ];
  if (*flag) return;
  const int tid = threadIdx.x;
  const int2 t = tasks[blockIdx.x];
  double *Ljk = S + (long)tid_map[(long)t.x * T + t.y] * (T64 * T64);
  load_tile(Ljk, sA, tid, false, T64);
  load_tile(Xinv + (long)t.y * T64 * T64, sB, tid, true, tile_lim(t.y, nR));   // sB[c][r] = X[r][c]
  __syncthreads();
  dbl4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  gemm64_nt(sA, sB, tid, acc);
  const int lim = tile_lim(t.x, nR);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int row, col;
      acc_pos(tid, q, reg, row, col);
      Ljk[row * T64 + col] = row < lim ? acc[q][reg] : 0.0;
    }
}

// Z_ik = - sum_{j in I_k} Z_ij G_jk for the tiles (i, k) of one level
__global__ __launch_bounds__(256) void k_selinv_off(const double *__restrict__ G, double *__restrict__ Z,
                                                    const int *__restrict__ tid_map, int T,
                                                    const int2 *__restrict__ gather, const int *__restrict__ gcol,
                                                    const int *__restrict__ gbeg, int g0,
                                                    const int *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) double sA[T64 * LQ];
  __shared__ __attribute__((aligned(16))) double sB[T64 * LQ];
  if (*flag) return;
  const int tid = threadIdx.x;
  const int g = g0 + blockIdx.x;
  const int2 t = gather[g];
  const int i = t.x, k = t.y;
  const int b = gcol[g];   // the column's position in bs_cols
  dbl4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int q = gbeg[b]; q < gbeg[b + 1]; ++q) {
    const int j = gather[q].x;
    if (q > gbeg[b]) __syncthreads();   // the previous product's fragments consumed
    // Z_ij: its own tile for i >= j, the transpose of Z_ji above the diagonal
    const double *Zij = Z + (long)tid_map[(long)(i >= j ? i : j) * T + (i >= j ? j : i)] * (T64 * T64);
    load_tile(Zij, sA, tid, i < j, T64);
    load_tile(G + (long)tid_map[(long)j * T + k] * (T64 * T64), sB, tid, true, T64);   // sB[c][r] = G[r][c]
    __syncthreads();
    gemm64_nt(sA, sB, tid, acc);
  }
  double *Zik = Z + (long)tid_map[(long)i * T + k] * (T64 * T64);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int row, col;
      acc_pos(tid, q, reg, row, col);
      Zik[row * T64 + col] = -acc[q][reg];
    }
}

// Z_kk = X_kk^T X_kk - sum_{j in I_k} G_jk^T Z_jk for the columns of one level:
// the lower triangle as computed, the upper its mirror
__global__ __launch_bounds__(256) void k_selinv_diag(const double *__restrict__ G, double *__restrict__ Z,
                                                     const int *__restrict__ tid_map, int T,
                                                     const double *__restrict__ Xinv, long nR,
                                                     const int *__restrict__ cols, const int2 *__restrict__ gather,
                                                     const int *__restrict__ gbeg, int b0,
                                                     const int *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) double sA[T64 * LQ];
  __shared__ __attribute__((aligned(16))) double sB[T64 * LQ];
  if (*flag) return;
  const int tid = threadIdx.x;
  const int b = b0 + blockIdx.x;
  const int k = cols[b];
  dbl4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  dbl4 sub[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  load_tile(Xinv + (long)k * T64 * T64, sA, tid, true, tile_lim(k, nR));   // sA[a][r] = X[r][a]
  __syncthreads();
  gemm64_nt(sA, sA, tid, acc);
  for (int q = gbeg[b]; q < gbeg[b + 1]; ++q) {
    const int j = gather[q].x;
    const long tj = (long)tid_map[(long)j * T + k] * (T64 * T64);
    __syncthreads();
    load_tile(G + tj, sA, tid, true, T64);   // sA[a][r] = G[r][a]
    load_tile(Z + tj, sB, tid, true, T64);   // sB[b][r] = Z[r][b]
    __syncthreads();
    gemm64_nt(sA, sB, tid, sub);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int row, col;
      acc_pos(tid, q, reg, row, col);
      sA[row * LQ + col] = acc[q][reg] - sub[q][reg];
    }
  __syncthreads();
  double *Zkk = Z + (long)tid_map[(long)k * T + k] * (T64 * T64);
#pragma unroll 4
  for (int m = 0; m < 16; ++m) {
    const int e = m * 256 + tid, r = e >> 6, c = e & 63;
    Zkk[e] = r >= c ? sA[r * LQ + c] : sA[c * LQ + r];
  }
}

// ---------------------------------------------------------------------------
// Marginal blocks of the covariance from Z (arslam_lm_covariance).

// Reduced-side blocks: thread (t, e) writes element e = 6 i + j of f-block t's
// 6x6 block, s_i s_j Z[row + i][row + j], the lower element for both (i, j)
// and (j, i); t == nt: var(f) from the camera's first row.  A block that is
// not on the reduced side gets -1.
__global__ void k_cov_fblocks(DevProblem P, const double *__restrict__ Z, const double *__restrict__ scale,
                              double *__restrict__ cov_f, double *__restrict__ var_f,
                              const int *__restrict__ flag) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id > 36L * P.nt) return;
  const bool bad = *flag != 0;
  if (id == 36L * P.nt) {
    *var_f = (P.cam_row < 0 || bad) ? -1.0 : scale[0] * scale[0] * z_elem(Z, P, P.cam_row, P.cam_row);
    return;
  }
  const int t = (int)(id / 36), e = (int)(id % 36), i = e / 6, j = e % 6;
  const int row = P.tag_row[t];
  if (row < 0 || bad) {
    cov_f[id] = -1.0;
    return;
  }
  const long sl = 3 + 6L * P.nc + 6L * t;
  const int hi = i >= j ? i : j, lo = i >= j ? j : i;
  cov_f[id] = scale[sl + hi] * scale[sl + lo] * z_elem(Z, P, row + hi, row + lo);
}

// Elimination of e-block c for the covariance, one wavefront each, by an
// orthogonal factorization of its scaled Jacobian columns E = Q R (modified
// Gram-Schmidt, every column orthogonalized twice) instead of the normal
// equations' U = E'E: with G = Q'F over the e-block's local f-side columns
// (the focal, then 6 per distinct f-block) its local reduced system is
//   F'F - G'G
// whose rounding error is not multiplied by cond(U), as that of
// F'F - W'U^{-1}W is (k_schur: fine for an LM step, ten times the normal
// equations' own error in a covariance).  Stored block-packed in the slab in
// k_schur's layout (schur_block_off; diagonal blocks whole, the rhs row zero)
// for k_schur_gather.  Kept for k_cov_eblocks: G (6 per local column, at
// Gb + 6 (c + 6 cap_blk_start[c])) and R (Rb + 36 c, upper triangle).
// Q lives in the global scratch Qb (6 per Jacobian row, e-block c's at
// 48 cap_start[c]); a lane only ever touches its own rows of it.
// A constant e-block has scale 0: Q = 0, G = 0, and its F'F goes in whole.
__global__ __launch_bounds__(kWave) void k_cov_schur(DevProblem P, const double *__restrict__ scale,
                                                     double *__restrict__ Qb, double *__restrict__ Gb,
                                                     double *__restrict__ Rb, int write_slab) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int o0 = P.cap_start[c], k = P.cap_start[c + 1] - o0;
  if (k == 0) return;
  const int R = 8 * k;
  const int b0 = P.cap_blk_start[c], nblk = P.cap_blk_start[c + 1] - b0;
  const int m = 1 + 6 * nblk;
  const long sc = 3 + 6L * c, st0 = 3 + 6L * P.nc;
  double *Q = Qb + 48L * o0;
  double *G = Gb + 6L * (c + 6L * b0);
  const double *jr = P.jrows + 8L * o0 * kJStored;
  for (int r = lane; r < R; r += kWave)
#pragma unroll
    for (int a = 0; a < 6; ++a) Q[6 * r + a] = jr[(long)jrow_col(1 + a) * R + r] * scale[sc + a];
  double Rq[6][6];
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) Rq[a][b] = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
      for (int b = 0; b < a; ++b) {
        double d = 0.0;
        for (int r = lane; r < R; r += kWave) d += Q[6 * r + b] * Q[6 * r + a];
        d = wave_sum64(d);
        Rq[b][a] += d;
        for (int r = lane; r < R; r += kWave) Q[6 * r + a] -= d * Q[6 * r + b];
      }
    double n2 = 0.0;
    for (int r = lane; r < R; r += kWave) n2 += Q[6 * r + a] * Q[6 * r + a];
    n2 = wave_sum64(n2);
    const double nrm = sqrt(n2);
    Rq[a][a] = nrm;
    const double inv = (n2 > 0.0 && n2 < INFINITY) ? 1.0 / nrm : 0.0;
    for (int r = lane; r < R; r += kWave) Q[6 * r + a] *= inv;
  }
  if (lane == 0)
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) Rb[36L * c + 6 * a + b] = Rq[a][b];
  __syncthreads();
  // F[r][col]: the focal column (col 0) on every row, column j of f-block u on
  // the rows of the observations whose block is u
  const double s0 = scale[0];
  for (int col = lane; col < m; col += kWave) {
    double g[6] = {0, 0, 0, 0, 0, 0};
    if (col == 0) {
      for (int r = 0; r < R; ++r) {
        const double f = jr[r] * s0;
#pragma unroll
        for (int a = 0; a < 6; ++a) g[a] += Q[6 * r + a] * f;
      }
    } else {
      const int u = (col - 1) / 6, j = (col - 1) % 6;
      const double *Fj = jr + (long)jrow_col(7 + j) * R;
      for (int q = 0; q < k; ++q) {
        if (P.obs_lblk[o0 + q] - 1 != u) continue;
        const double st = scale[st0 + 6L * P.obs_tag[o0 + q] + j];
        for (int r = 8 * q; r < 8 * q + 8; ++r) {
          const double f = Fj[r] * st;
#pragma unroll
          for (int a = 0; a < 6; ++a) g[a] += Q[6 * r + a] * f;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) G[6 * col + a] = g[a];
  }
  __syncthreads();
  if (!write_slab) return;
  // (p, q) of the local reduced system, q in p's block row: F_p'F_q (nonzero
  // for the focal against anything and inside one f-block: two f-blocks share
  // no row) minus G_p'G_q; the same bits for (p, q) and (q, p)
  auto entry = [&](int p, int q) -> double {
    double ff = 0.0;
    if (p == 0 && q == 0) {
      for (int r = 0; r < R; ++r) ff += (jr[r] * s0) * (jr[r] * s0);
    } else if (p == 0 || q == 0 || (p - 1) / 6 == (q - 1) / 6) {
      const int x = p == 0 ? q : p, y = p == 0 ? p : q;   // x: a block column; y: the focal or one of the same block
      const int u = (x - 1) / 6, jx = (x - 1) % 6, jy = y == 0 ? 0 : (y - 1) % 6;
      const double *Fx = jr + (long)jrow_col(7 + jx) * R, *Fy = jr + (long)jrow_col(7 + jy) * R;
      for (int o = 0; o < k; ++o) {
        if (P.obs_lblk[o0 + o] - 1 != u) continue;
        const long sl = st0 + 6L * P.obs_tag[o0 + o];
        const double sx = scale[sl + jx], sy = y == 0 ? s0 : scale[sl + jy];
        for (int r = 8 * o; r < 8 * o + 8; ++r) ff += (Fx[r] * sx) * ((y == 0 ? jr[r] : Fy[r]) * sy);
      }
    }
    double gg = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) gg += G[6 * p + a] * G[6 * q + a];
    return ff - gg;
  };
  double *out = P.slab + P.cap_off[c];
  for (int U = 0; U <= nblk + 1; ++U) {
    const int sU = schur_blk_size(U, nblk), p0U = schur_blk_start(U, nblk), ncol = p0U + sU;
    double *dst = out + schur_block_off(U, 0, nblk);
    for (int q = lane; q < ncol; q += kWave) {
      const int V = schur_blk(q < m ? q : m, m), sV = schur_blk_size(V, nblk), q0V = schur_blk_start(V, nblk);
      for (int i = 0; i < sU; ++i)
        dst[(long)sU * q0V + i * sV + (q - q0V)] = U == nblk + 1 ? 0.0 : entry(p0U + i, q);
    }
  }
}

// Eliminated blocks, one wavefront per e-block c, from k_cov_schur's G and R:
//   C_c = R^{-1} (I + sum_{p,q} G_p Z_pq G_q^T) R^{-T}
// over the e-block's local f-side columns p, q (= U^{-1} + Y Z Y^T with
// Y = U^{-1} W, without forming U), then unscaled.  Columns of constant
// f-blocks (no reduced row) are skipped: their G is 0.  The local Z is never
// staged: lane p walks row p of it against G (column order), the lanes'
// partial blocks are added in lane order.  One triangle is computed and
// mirrored.  status[c]: 0 computed, 1 not a free block in use, 2 R is singular
// (or not finite).
__global__ __launch_bounds__(kWave) void k_cov_eblocks(DevProblem P, const double *__restrict__ Z,
                                                       const double *__restrict__ scale,
                                                       const double *__restrict__ Gb, const double *__restrict__ Rb,
                                                       double *__restrict__ cov_e, int *__restrict__ status,
                                                       const int *__restrict__ flag) {
  __shared__ double Ri[36], Ms[36], part[kWave][21];
  __shared__ int ok;
  const int c = blockIdx.x, lane = threadIdx.x;
  const int o0 = P.cap_start[c], k = P.cap_start[c + 1] - o0;
  const long sc = 3 + 6L * c;
  double *out = cov_e + 36L * c;
  if (k == 0 || !P.slot_free[sc] || *flag != 0) {
    if (lane < 36) out[lane] = -1.0;
    if (lane == 0) status[c] = (k == 0 || !P.slot_free[sc]) ? 1 : 2;
    return;
  }
  const int b0 = P.cap_blk_start[c], nblk = P.cap_blk_start[c + 1] - b0;
  const int m = 1 + 6 * nblk;
  const double *G = Gb + 6L * (c + 6L * b0);
  if (lane == 0) {
    // R^{-1} (upper triangular), one lane
    const double *Rq = Rb + 36L * c;
    bool good = true;
    for (int a = 0; a < 6; ++a) good = good && Rq[7 * a] > 0.0 && Rq[7 * a] < INFINITY;
    for (int col = 0; col < 6; ++col)
      for (int a = 5; a >= 0; --a) {
        double v = a == col ? 1.0 : 0.0;
        for (int p = a + 1; p <= col; ++p) v -= Rq[6 * a + p] * Ri[6 * p + col];
        Ri[6 * a + col] = a <= col ? v / Rq[7 * a] : 0.0;
        good = good && isfinite(Ri[6 * a + col]);
      }
    ok = good ? 1 : 0;
  }
  __syncthreads();
  if (!ok) {
    if (lane < 36) out[lane] = -1.0;
    if (lane == 0) status[c] = 2;
    return;
  }
  // reduced row of local column col (-1: a constant f-block's, or no free focal)
  auto col_row = [&](int col) -> long {
    if (col == 0) return P.cam_row;
    const int r = P.tag_row[P.blk_tag[b0 + (col - 1) / 6]];
    return r < 0 ? -1 : r + (col - 1) % 6;
  };
  double acc[21];
#pragma unroll
  for (int e = 0; e < 21; ++e) acc[e] = 0.0;
  for (int p = lane; p < m; p += kWave) {
    const long rp = col_row(p);
    if (rp < 0) continue;
    double v[6] = {0, 0, 0, 0, 0, 0};   // v = Z[rp][:] G^T
    for (int q = 0; q < m; ++q) {
      const long rq = col_row(q);
      if (rq < 0) continue;
      const double z = z_elem(Z, P, rp, rq);
#pragma unroll
      for (int a = 0; a < 6; ++a) v[a] += z * G[6 * q + a];
    }
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) acc[e++] += G[6 * p + a] * v[b];
  }
#pragma unroll
  for (int e = 0; e < 21; ++e) part[lane][e] = acc[e];
  __syncthreads();
  if (lane < 21) {
    double s = 0.0;
    for (int l = 0; l < kWave; ++l) s += part[l][lane];
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= lane) ++a;
    const int b = lane - a * (a + 1) / 2;
    const double v = (a == b ? 1.0 : 0.0) + s;
    Ms[6 * a + b] = v;
    Ms[6 * b + a] = v;
  }
  __syncthreads();
  if (lane < 21) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= lane) ++i;
    const int j = lane - i * (i + 1) / 2;
    double v = 0.0;
    for (int a = 0; a < 6; ++a) {
      double t = 0.0;
      for (int b = 0; b < 6; ++b) t += Ms[6 * a + b] * Ri[6 * j + b];
      v += Ri[6 * i + a] * t;
    }
    v *= scale[sc + i] * scale[sc + j];
    out[6 * i + j] = v;
    out[6 * j + i] = v;
  }
  if (lane == 0) status[c] = 0;
}

}  // namespace

void launch_cov_schur(const DevProblem &P, const double *scale, double *Qb, double *Gb, double *Rb, bool write_slab,
                      hipStream_t s) {
  if (P.nc > 0)
    hipLaunchKernelGGL(k_cov_schur, dim3((unsigned)P.nc), dim3(kWave), 0, s, P, scale, Qb, Gb, Rb, write_slab ? 1 : 0);
}

void launch_cov_blocks(const DevProblem &P, const double *Z, const double *scale, const double *Gb, const double *Rb,
                       double *cov_e, int *status_e, double *cov_f, double *var_f, const int *flag, hipStream_t s) {
  if (P.nc > 0)
    hipLaunchKernelGGL(k_cov_eblocks, dim3((unsigned)P.nc), dim3(kWave), 0, s, P, Z, scale, Gb, Rb, cov_e, status_e,
                       flag);
  const long nf = 36L * P.nt + 1;
  hipLaunchKernelGGL(k_cov_fblocks, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, P, Z, scale, cov_f, var_f,
                     flag);
}

void selinv_plan_build(const LltPlan &P, SelinvPlan &sp, hipStream_t s) {
  selinv_plan_free(sp);
  const std::vector<int> &gbeg = P.h_gbeg;
  std::vector<int> gcol(std::max<size_t>(P.h_gather.size(), 1), 0);
  sp.n_products = 0;
  for (size_t b = 0; b + 1 < gbeg.size(); ++b) {
    const long m = gbeg[b + 1] - gbeg[b];
    for (int g = gbeg[b]; g < gbeg[b + 1]; ++g) gcol[g] = (int)b;
    sp.n_products += m + m * m + 1 + m;   // G, the off-diagonal Z, X^T X and the diagonal's sum
  }
  if (hipMalloc(&sp.gcol, gcol.size() * sizeof(int)) != hipSuccess) throw std::runtime_error("selinv: hipMalloc");
  if (hipMemcpyAsync(sp.gcol, gcol.data(), gcol.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    selinv_plan_free(sp);
    throw std::runtime_error("selinv: hipMemcpy");
  }
}

void selinv_plan_free(SelinvPlan &sp) {
  if (sp.gcol) (void)hipFree(sp.gcol);
  sp.gcol = nullptr;
  sp.n_products = 0;
}

void launch_selinv(const LltPlan &P, const SelinvPlan &sp, double *S, long nR, double *Z, const int *flag,
                   hipStream_t s) {
  const double *Xinv = P.ldiag + (long)P.T * T64 * T64;
  const int ng_all = (int)P.h_gather.size();
  if (ng_all > 0)
    hipLaunchKernelGGL(k_selinv_g, dim3((unsigned)ng_all), dim3(256), 0, s, S, P.tile_id, P.T, Xinv, nR, P.bs_gather,
                       flag);
  const int nlev = (int)P.h_bs_off.size() - 1;
  for (int l = 0; l < nlev; ++l) {
    const int g0 = P.h_bsg_off[l], ng = P.h_bsg_off[l + 1] - g0;
    if (ng > 0)
      hipLaunchKernelGGL(k_selinv_off, dim3((unsigned)ng), dim3(256), 0, s, S, Z, P.tile_id, P.T, P.bs_gather,
                         sp.gcol, P.bs_gbeg, g0, flag);
    const int b0 = P.h_bs_off[l], nc = P.h_bs_off[l + 1] - b0;
    if (nc > 0)
      hipLaunchKernelGGL(k_selinv_diag, dim3((unsigned)nc), dim3(256), 0, s, S, Z, P.tile_id, P.T, Xinv, nR,
                         P.bs_cols, P.bs_gather, P.bs_gbeg, b0, flag);
  }
}

}  // namespace arslam
