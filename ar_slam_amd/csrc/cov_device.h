// cov_device.h -- the small device helpers the covariance's block kernels
// share (selinv.hip, cov_pairs.hip, cov_lens.hip): an element of the selected
// inverse, a wavefront sum, an element of a right-hand-side panel, the inverse
// of an e-block's R and the reduced row of an e-block's local column.
//
// Everything sits in an anonymous namespace, as in lm_rows.h: every translation
// unit gets its own internal copy, so a kernel's machine code does not depend on
// which kernels of another file call the same helper.
#pragma once
#include "llt_tile.h"
#include "lm_cov.h"

namespace arslam {

namespace {

// Z[r][c] of the selected inverse (either triangle: the stored tile is (max, min))
__device__ __forceinline__ double z_elem(const double *__restrict__ Z, const DevProblem &P, long r, long c) {
  const long a = r >= c ? r : c, b = r >= c ? c : r;
  const int id = P.tile_id[(a >> 6) * P.T + (b >> 6)];
  // (every pair of one e-block's f-blocks is an assembled tile; a pair outside the factor has no Z)
  return id < 0 ? __builtin_nan("") : Z[(long)id * 4096 + (a & 63) * 64 + (b & 63)];
}

// sum over the wavefront, the same bits in every lane (xor butterfly)
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// element (r, c) of panel column block `slot` of a batch of panels
__device__ __forceinline__ double *panel_elem(double *B, int T, int slot, long r, int c) {
  return B + ((long)(slot / kCovPanelBlocks) * T + (r >> 6)) * (T64 * T64) + (r & 63) * T64 +
         (slot % kCovPanelBlocks) * 6 + c;
}

// Ri = R^{-1} of e-block c's 6x6 upper-triangular R (k_cov_schur), one lane;
// false when R is singular or not finite
__device__ bool r_inverse(const double *__restrict__ Rq, double *Ri) {
  bool good = true;
  for (int a = 0; a < 6; ++a) good = good && Rq[7 * a] > 0.0 && Rq[7 * a] < INFINITY;
  for (int col = 0; col < 6; ++col)
    for (int a = 5; a >= 0; --a) {
      double v = a == col ? 1.0 : 0.0;
      for (int p = a + 1; p <= col; ++p) v -= Rq[6 * a + p] * Ri[6 * p + col];
      Ri[6 * a + col] = a <= col ? v / Rq[7 * a] : 0.0;
      good = good && isfinite(Ri[6 * a + col]);
    }
  return good;
}

// reduced row of local column col of e-block c (the focal, then 6 per distinct
// f-block); -1: a constant f-block's, or no free focal
__device__ __forceinline__ long local_col_row(const DevProblem &P, int b0, int col) {
  if (col == 0) return P.cam_row;
  const int r = P.tag_row[P.blk_tag[b0 + (col - 1) / 6]];
  return r < 0 ? -1 : r + (col - 1) % 6;
}

}  // namespace

}  // namespace arslam
