// cov_lens.hip -- the covariance with the camera's l1, l2 estimated (the
// handle's "estimate the distortion" switch on a loaded problem with a free
// camera; arslam_lm_covariance_lens, arslam_lm_covariance_pairs_lens; fp64,
// gfx950).
//
// The orthogonal elimination (k_cov_schur, selinv.hip) forms an e-block's local
// reduced system over [f | 6 per distinct f-block] in k_schur's slab layout,
// which has no room for two more columns.  As in the LM step (lm_schur_cam.hip)
// they are a border computed beside it.  With the e-block's scaled rows
// [f | E | F] (jrows), E = Q R, and their l columns L_a (DevCamL::jrows_l),
//   G_la = Q'L_a,   border(a, q) = L_a'F_q - G_la'G_q
// for every local column q (f, the tag columns, l_b with b <= a: F_q = L_b;
// G_q is k_cov_schur's); the rhs entry is 0, as k_cov_schur's rhs row is.
// L_a'F_q runs over the rows where F_q lives.  A constant e-block has scale 0:
// Q = 0, every G = 0, and L_a'F_q goes in whole.
//
// k_cov_schur_cam, one wavefront per e-block after k_cov_schur, stores the
// border in k_schur_cam's layout (cam_slab_off, ld = m + 3), so
// k_schur_cam_gather assembles it unchanged, and keeps G_la (12 per e-block)
// for the block kernels.  Those are k_cov_eblocks, k_cov_fblocks,
// k_cov_pair_rhs and k_cov_pair_blocks with the camera three wide: an
// e-block's local columns gain l1, l2 (reduced rows cam_row + 1, cam_row + 2,
// G_la), the camera's block is 3x3 and its right-hand side three unit columns.
//
// Plain launches; every sum in a fixed order (rows by lane stride and one xor
// butterfly, or one lane in row order), no atomics.
#include "cov_device.h"
#include "lm_launch.h"

namespace arslam {

namespace {

__global__ __launch_bounds__(kWave) void k_cov_schur_cam(DevProblem P, DevCamL CL, const double *__restrict__ scale,
                                                         const double *__restrict__ Qb, const double *__restrict__ Gb,
                                                         double *__restrict__ Glb) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int o0 = P.cap_start[c], k = P.cap_start[c + 1] - o0;
  const int b0 = P.cap_blk_start[c], nblk = P.cap_blk_start[c + 1] - b0;
  const int m = 1 + 6 * nblk, ld = m + 3;
  double *out = CL.cam_slab + cam_slab_off(P, c);
  double *Gl = Glb + 12L * c;
  if (k == 0) {   // (k_cov_schur leaves it nothing; the gather's capture-wide sums read every e-block's border)
    for (int e = lane; e < 2 * ld; e += kWave) out[e] = 0.0;
    if (lane < 12) Gl[lane] = 0.0;
    return;
  }
  const int R = 8 * k;
  const long st0 = 3 + 6L * P.nc;
  const double *Q = Qb + 48L * o0;
  const double *G = Gb + 6L * (c + 6L * b0);
  const double *jr = P.jrows + 8L * o0 * kJStored;
  const double *lb = CL.jrows_l + 16L * o0;
  const double s0 = scale[0], sl0 = scale[1], sl1 = scale[2];
  // G_la = Q'L_a and the capture-wide products (l1, f), (l2, f), (l1, l1), (l2, l1), (l2, l2)
  double gl[12], tot[5];
#pragma unroll
  for (int e = 0; e < 12; ++e) gl[e] = 0.0;
#pragma unroll
  for (int e = 0; e < 5; ++e) tot[e] = 0.0;
  for (int r = lane; r < R; r += kWave) {
    const double L0 = lb[r] * sl0, L1 = lb[R + r] * sl1, f = jr[r] * s0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double q = Q[6 * r + i];
      gl[i] += q * L0;
      gl[6 + i] += q * L1;
    }
    tot[0] += L0 * f;
    tot[1] += L1 * f;
    tot[2] += L0 * L0;
    tot[3] += L1 * L0;
    tot[4] += L1 * L1;
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) gl[e] = wave_sum64(gl[e]);
#pragma unroll
  for (int e = 0; e < 5; ++e) tot[e] = wave_sum64(tot[e]);
  // the tag columns: lane per column, the rows of its f-block's observations in order
  for (int col = 1 + lane; col < m; col += kWave) {
    const int u = (col - 1) / 6, j = (col - 1) % 6;
    const double *Fj = jr + (long)jrow_col(7 + j) * R;
    double ff0 = 0.0, ff1 = 0.0;
    for (int q = 0; q < k; ++q) {
      if (P.obs_lblk[o0 + q] - 1 != u) continue;
      const double st = scale[st0 + 6L * P.obs_tag[o0 + q] + j];
      for (int r = 8 * q; r < 8 * q + 8; ++r) {
        const double f = Fj[r] * st;
        ff0 += (lb[r] * sl0) * f;
        ff1 += (lb[R + r] * sl1) * f;
      }
    }
    double gg0 = 0.0, gg1 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double g = G[6 * col + i];
      gg0 += gl[i] * g;
      gg1 += gl[6 + i] * g;
    }
    out[col] = ff0 - gg0;
    out[ld + col] = ff1 - gg1;
  }
  if (lane == 0) {
    double gf0 = 0.0, gf1 = 0.0, g00 = 0.0, g10 = 0.0, g11 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      Gl[i] = gl[i];
      Gl[6 + i] = gl[6 + i];
      gf0 += gl[i] * G[i];
      gf1 += gl[6 + i] * G[i];
      g00 += gl[i] * gl[i];
      g10 += gl[6 + i] * gl[i];
      g11 += gl[6 + i] * gl[6 + i];
    }
    out[0] = tot[0] - gf0;
    out[ld] = tot[1] - gf1;
    out[m] = tot[2] - g00;
    out[m + 1] = 0.0;   // (l1, l2): the lower triangle holds (l2, l1)
    out[ld + m] = tot[3] - g10;
    out[ld + m + 1] = tot[4] - g11;
    out[m + 2] = 0.0;   // the rhs
    out[ld + m + 2] = 0.0;
  }
}

// k_cov_fblocks with the camera's 3x3 block [f, l1, l2] in place of var(f):
// thread 36 nt + 3 i + j writes s_i s_j Z[cam_row + i][cam_row + j], the lower
// element for both (i, j) and (j, i).
__global__ void k_cov_fblocks_lens(DevProblem P, const double *__restrict__ Z, const double *__restrict__ scale,
                                   double *__restrict__ cov_f, double *__restrict__ cov_cam,
                                   const int *__restrict__ flag) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= 36L * P.nt + 9) return;
  const bool bad = *flag != 0;
  if (id >= 36L * P.nt) {
    const int e = (int)(id - 36L * P.nt), i = e / 3, j = e % 3;
    const int hi = i >= j ? i : j, lo = i >= j ? j : i;
    cov_cam[e] = (P.cam_row < 0 || bad) ? -1.0 : scale[hi] * scale[lo] * z_elem(Z, P, P.cam_row + hi, P.cam_row + lo);
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

// reduced row and G of local column col of e-block c with the two l columns
// after the m = 1 + 6 nblk columns of k_cov_schur
__device__ __forceinline__ long lens_col_row(const DevProblem &P, int b0, int m, int col) {
  return col >= m ? (long)P.cam_row + 1 + (col - m) : local_col_row(P, b0, col);
}
__device__ __forceinline__ const double *lens_col_g(const double *G, const double *Gl, int m, int col) {
  return col >= m ? Gl + 6 * (col - m) : G + 6 * col;
}

// k_cov_eblocks over the local columns [f | 6 per distinct f-block | l1 | l2]:
//   C_c = R^{-1} (I + sum_{p,q} G_p Z_pq G_q^T) R^{-T}
__global__ __launch_bounds__(kWave) void k_cov_eblocks_lens(DevProblem P, const double *__restrict__ Z,
                                                            const double *__restrict__ scale,
                                                            const double *__restrict__ Gb, const double *__restrict__ Rb,
                                                            const double *__restrict__ Glb, double *__restrict__ cov_e,
                                                            int *__restrict__ status, const int *__restrict__ flag) {
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
  const int m = 1 + 6 * nblk, ml = m + 2;
  const double *G = Gb + 6L * (c + 6L * b0);
  const double *Gl = Glb + 12L * c;
  if (lane == 0) ok = r_inverse(Rb + 36L * c, Ri) ? 1 : 0;
  __syncthreads();
  if (!ok) {
    if (lane < 36) out[lane] = -1.0;
    if (lane == 0) status[c] = 2;
    return;
  }
  double acc[21];
#pragma unroll
  for (int e = 0; e < 21; ++e) acc[e] = 0.0;
  for (int p = lane; p < ml; p += kWave) {
    const long rp = lens_col_row(P, b0, m, p);
    if (rp < 0) continue;
    double v[6] = {0, 0, 0, 0, 0, 0};   // v = Z[rp][:] G^T
    for (int q = 0; q < ml; ++q) {
      const long rq = lens_col_row(P, b0, m, q);
      if (rq < 0) continue;
      const double z = z_elem(Z, P, rp, rq);
      const double *gq = lens_col_g(G, Gl, m, q);
#pragma unroll
      for (int a = 0; a < 6; ++a) v[a] += z * gq[a];
    }
    const double *gp = lens_col_g(G, Gl, m, p);
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) acc[e++] += gp[a] * v[b];
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

// k_cov_pair_rhs with the camera three wide: unit columns at cam_row + 0..2 for
// the camera, and an e-block's -(R^{-1} G)^T over its l columns too.
__global__ __launch_bounds__(kWave) void k_cov_pair_rhs_lens(DevProblem P, const double *__restrict__ Gb,
                                                             const double *__restrict__ Rb,
                                                             const double *__restrict__ Glb,
                                                             const int2 *__restrict__ rhs, double *__restrict__ B,
                                                             int T) {
  __shared__ double Ri[36];
  __shared__ int ok;
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int2 blk = rhs[slot];
  if (blk.x == kCovFocal) {
    if (lane < 3 && P.cam_row >= 0) *panel_elem(B, T, slot, P.cam_row + lane, lane) = 1.0;
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
  const double *Gl = Glb + 12L * c;
  for (int p = lane; p < m + 2; p += kWave) {
    const long row = lens_col_row(P, b0, m, p);
    if (row < 0) continue;
    const double *gp = lens_col_g(G, Gl, m, p);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double y = 0.0;
#pragma unroll
      for (int q = a; q < 6; ++q) y += Ri[6 * a + q] * gp[q];
      *panel_elem(B, T, slot, row, a) = -y;
    }
  }
}

// k_cov_pair_blocks with the camera three wide (three rows as a, three columns
// as b, the rest 0) and the e-blocks' l columns.
__global__ __launch_bounds__(kWave) void k_cov_pair_blocks_lens(DevProblem P, const double *__restrict__ X, int T,
                                                                const double *__restrict__ scale,
                                                                const double *__restrict__ Gb,
                                                                const double *__restrict__ Rb,
                                                                const double *__restrict__ Glb,
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
  const int na = t.role_a == kCovFocal ? 3 : 6, nb = t.role_b == kCovFocal ? 3 : 6;
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
    const double *Gl = Glb + 12L * c;
    if (lane < 36) {   // V = G X_b[loc(a), :], the local columns in order
      double s = 0.0;
      if (Xs && j < nb)
        for (int p = 0; p < m + 2; ++p) {
          const long row = lens_col_row(P, b0, m, p);
          if (row >= 0) s += lens_col_g(G, Gl, m, p)[i] * xel(row);
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

void launch_cov_schur_cam(const DevProblem &P, const DevCamL &cl, const double *scale, const double *Qb,
                          const double *Gb, double *Glb, hipStream_t s) {
  if (P.nc > 0 && P.cam_row >= 0)
    hipLaunchKernelGGL(k_cov_schur_cam, dim3((unsigned)P.nc), dim3(kWave), 0, s, P, cl, scale, Qb, Gb, Glb);
}

void launch_cov_blocks_lens(const DevProblem &P, const double *Z, const double *scale, const double *Gb,
                            const double *Rb, const double *Glb, double *cov_e, int *status_e, double *cov_f,
                            double *cov_cam, const int *flag, hipStream_t s) {
  if (P.nc > 0)
    hipLaunchKernelGGL(k_cov_eblocks_lens, dim3((unsigned)P.nc), dim3(kWave), 0, s, P, Z, scale, Gb, Rb, Glb, cov_e,
                       status_e, flag);
  const long nf = 36L * P.nt + 9;
  hipLaunchKernelGGL(k_cov_fblocks_lens, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, P, Z, scale, cov_f,
                     cov_cam, flag);
}

void launch_cov_pair_rhs_lens(const DevProblem &P, const double *Gb, const double *Rb, const double *Glb,
                              const int2 *rhs, int n_rhs, double *B, hipStream_t s) {
  if (n_rhs > 0)
    hipLaunchKernelGGL(k_cov_pair_rhs_lens, dim3((unsigned)n_rhs), dim3(kWave), 0, s, P, Gb, Rb, Glb, rhs, B, P.T);
}

void launch_cov_pair_blocks_lens(const DevProblem &P, const double *X, const double *scale, const double *Gb,
                                 const double *Rb, const double *Glb, const CovPairTask *tasks, int n_tasks,
                                 double *out, int *status, const int *flag, hipStream_t s) {
  if (n_tasks > 0)
    hipLaunchKernelGGL(k_cov_pair_blocks_lens, dim3((unsigned)n_tasks), dim3(kWave), 0, s, P, X, P.T, scale, Gb, Rb,
                       Glb, tasks, out, status, flag);
}

}  // namespace arslam
