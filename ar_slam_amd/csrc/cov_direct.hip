// cov_direct.hip -- the covariance's elimination over a direct group of the
// mixed e-block set (MixedProblem, kMixDirect; the anchored covariance forms,
// arslam_lm_covariance_anchored; fp64, gfx950).
//
// A direct group holds the residuals of one capture on the reduced side whose
// tag is on the reduced side too: nothing is eliminated, there is no Q, G or R.
// Its local system is the plain F'F of the scaled columns
//   [f | 6 per distinct tag | own pose | rhs = 0]
// in k_schur's slab layout (schur_block_off; the block order of
// store_direct_group), so k_schur_gather assembles it unchanged.  The group's
// rows are in e|f order with the own pose in the e columns (jrows columns
// 1..6): local block nblk - 1 spans every row of the group, so unlike the
// f-blocks of an eliminated group (k_cov_schur's entry()) it shares rows with
// each tag block and with the focal.  Its Jacobi scale comes from the aliased
// f-block's slots: the group's own slot is a copy the caller may have zeroed.
//
// k_cov_direct, one wavefront per direct group, runs after k_cov_schur on the
// same stream and stores the group's whole slab slot.  Every entry is one
// lane's sum over the rows in row order, the product taken with the smaller
// local column first: (p, q) and (q, p) are the same bits, call after call.
#include "cov_device.h"
#include "lm_launch.h"

namespace arslam {

namespace {

__global__ __launch_bounds__(kWave) void k_cov_direct(DevProblem P, const double *__restrict__ scale,
                                                      const int *__restrict__ groups) {
  const int c = groups[blockIdx.x], lane = threadIdx.x;
  if (c < 0 || c >= P.nc || !P.cap_kind || P.cap_kind[c] != kMixDirect) return;
  const int o0 = P.cap_start[c], k = P.cap_start[c + 1] - o0;
  const int b0 = P.cap_blk_start[c], nblk = P.cap_blk_start[c + 1] - b0;
  if (k == 0 || nblk < 1) return;
  const int R = 8 * k;
  const int m = 1 + 6 * nblk, own = nblk - 1;
  const long st0 = 3 + 6L * P.nc;
  const long own_sl = st0 + 6L * P.blk_tag[b0 + own];
  const double *jr = P.jrows + 8L * o0 * kJStored;
  const double s0 = scale[0];
  // the scaled local column p on row r of observation o
  auto colv = [&](int p, int o, int r) -> double {
    if (p == 0) return jr[r] * s0;
    const int u = (p - 1) / 6, j = (p - 1) % 6;
    if (u == own) return jr[(long)jrow_col(1 + j) * R + r] * scale[own_sl + j];
    return jr[(long)jrow_col(7 + j) * R + r] * scale[st0 + 6L * P.obs_tag[o0 + o] + j];
  };
  // the tag block whose observations' rows column p lives on; -1: every row (the focal, the own pose)
  auto rows_of = [&](int p) -> int {
    const int u = p == 0 ? own : (p - 1) / 6;
    return u == own ? -1 : u;
  };
  auto entry = [&](int p, int q) -> double {
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    const int tl = rows_of(lo), th = rows_of(hi);
    if (tl >= 0 && th >= 0 && tl != th) return 0.0;   // two tag blocks share no row
    const int need = tl >= 0 ? tl : th;
    double ff = 0.0;
    for (int o = 0; o < k; ++o) {
      if (need >= 0 && P.obs_lblk[o0 + o] - 1 != need) continue;
      for (int r = 8 * o; r < 8 * o + 8; ++r) ff += colv(lo, o, r) * colv(hi, o, r);
    }
    return ff;
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

}  // namespace

void launch_cov_direct(const DevProblem &P, const double *scale, const int *groups, int n_groups, hipStream_t s) {
  if (n_groups > 0)
    hipLaunchKernelGGL(k_cov_direct, dim3((unsigned)n_groups), dim3(kWave), 0, s, P, scale, groups);
}

}  // namespace arslam
