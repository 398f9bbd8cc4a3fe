// lm_rows.h -- the device helpers that the LM stages' kernels share
// (lm_linearize.hip, lm_schur.hip, lm_step.hip, lm_reduce.hip; debug_rows.hip
// for the corrector): the slots and kinds of a capture, its Jacobian rows and
// their stored copy (DevProblem::jrows), the two instances of a per-capture
// kernel, and the wave levels of a block's tree reduction.
//
// One 64-lane wavefront per capture (the eliminated Schur e-block).  Lane l
// of a 64-row chunk owns residual row l = 8*obs + 2*corner + {x,y} of that
// capture's observations, so the k = 8 observations of a synthetic capture
// are exactly one wave.  Each lane evaluates its row of the reference's
// residual (projectCorner, ar_slam_util.cpp:131-172; ArucoReprojectionError
// :198-211) and the analytic Jacobian into LDS
// (fill_rows).
//
// Everything sits in an anonymous namespace, as in llt_tile.h: every
// translation unit gets its own internal copy, all of it forceinline, so a
// kernel's machine code does not depend on which other kernels of its file
// call the same helper.
#pragma once
#include "lm_problem.h"
#include "loss.h"
#include "projection.h"

namespace arslam {

namespace {

__device__ __forceinline__ long slot_cap(const DevProblem &P, int c) { return 3 + 6L * c; }
__device__ __forceinline__ long slot_tag(const DevProblem &P, int t) { return 3 + 6L * P.nc + 6L * t; }

// does group c evaluate its residuals with the two poses exchanged (its e-block is a tag)?
__device__ __forceinline__ bool group_swapped(const DevProblem &P, int c) {
  return P.cap_kind ? P.cap_kind[c] == kMixTag : P.swap_roles != 0;
}
// a direct group of the mixed e-set (its own pose stays on the reduced side)?
__device__ __forceinline__ bool group_direct(const DevProblem &P, int c) {
  return P.cap_kind && P.cap_kind[c] == kMixDirect;
}

__device__ __forceinline__ double lm_d2(const double *diag, long slot, double radius) {
  const double d = sqrt(diag[slot] / radius);   // lm_diagonal_ = sqrt(diag / radius)
  return d * d;
}

// Ceres' corrector (corrector.cc, alpha = 0: every loss of loss.h has
// rho'' <= 0) on one row of an observation whose 8 rows sit in 8 consecutive
// lanes: r and its 13 Jacobian entries times sqrt(rho'(s)), s = |r|^2 over
// the 8 rows.  Returns rho(s), the same in the 8 lanes.
// (w_out: also the factor itself, for the columns the caller keeps beside J)
__device__ __forceinline__ double robustify_row(int kind, double a, double &r, double J[13],
                                                double *w_out = nullptr) {
  const double s = obs_sum8(r * r);
  double rho, rho1;
  loss_eval(kind, a, s, &rho, &rho1);
  const double w = sqrt(rho1);
  if (w_out) *w_out = w;
#pragma unroll
  for (int j = 0; j < 13; ++j) J[j] *= w;
  r *= w;
  return rho;
}

// Fill LDS rows [nr][kRowStride] with rows [row0, row0 + nr) of capture c
// (nrows rows in all, observations from o0): 13 Jacobian entries (scaled by
// the Jacobi scale if scale != nullptr) and the residual in column 13.
// With gout, the unscaled rows are also stored there column-major per capture
// (entry (row, j) at gout + 8 o0 kJStored + jrow_col(j) nrows + row, the
// translation columns once): the Schur and back-substitution passes at the
// same point reload them instead of re-evaluating the projection.
// kLoss: the rows are the corrected ones, sqrt(rho') (J | r) per observation
// (robustify_row), in LDS and in gout alike; with ocost, observation q of the
// chunk also leaves its cost rho(s) / 2 in ocost[q] (from the corrected
// residuals it would be rho' s / 2).
// kSized: the observation's tag side comes from DevProblem::obs_size; else
// every tag has the default side, a constant of the code.
// kDist: the rows of the radial camera model, l1 and l2 from camera slots 1
// and 2 of x (held: they never move, so a capture's rows are consistent over a
// solve); else the pinhole's.  kDist = 2 (the handle's "estimate the distortion"
// switch, DevCamL::jrows_l = lout): the radial rows, and the row's two l columns,
// d r / d l1 and d r / d l2 (corrected like the rest of the row), stored
// column-major per capture in lout ((row, a) at 16 o0 + a nrows
// + row); lsum then gets the lane's row's J_l1 r, J_l2 r, J_l1^2, J_l2^2 (zeros
// for a lane without a row): the capture's l gradient and column-norm terms.
template <bool kLoss = false, bool kSized = false, int kDist = 0>
__device__ __forceinline__ void fill_rows(const DevProblem &P, const double *x, const double *scale, int c,
                          int o0, int row0, int nr, int nrows, double *rows, double *gout = nullptr,
                          double *ocost = nullptr, double *lsum = nullptr, double *lout = nullptr) {
  if (kDist == 2) lsum[0] = lsum[1] = lsum[2] = lsum[3] = 0.0;
  const double *cam = x;
  const double *cap = x + slot_cap(P, c);
  for (int lr = threadIdx.x; lr < nr; lr += kWave) {
    const int row = row0 + lr;
    const int q = row >> 3, corner = (row >> 1) & 3, comp = row & 1;
    const int obs = o0 + q;
    const int t = P.obs_tag[obs];
    const double *tag = x + slot_tag(P, t);
    double J[13];
    // (tag elimination: the e-block is the problem's tag -- projectCorner
    // still takes the capture first; the Jacobian halves come back as e|f)
    const bool sw = group_swapped(P, c);
    const double half = kSized ? 0.5 * P.obs_size[obs] : kArucoHalf;
    double Jl[2], w = 1.0;
    double r = residual_jacobian_row<kDist != 0>(cam, sw ? tag : cap, sw ? cap : tag, half, corner, comp,
                                                 P.corners[8L * obs + 2 * corner + comp], J,
                                                 kDist == 2 ? Jl : nullptr);
    if (kLoss) {
      // (nr is a multiple of 8: an observation's 8 lanes are in the loop together)
      const double rho = robustify_row(P.obs_loss_kind[obs], P.obs_loss_a[obs], r, J, kDist == 2 ? &w : nullptr);
      if (ocost && (lr & 7) == 0) ocost[lr >> 3] = 0.5 * rho;
    }
    if (kDist == 2) {
      if (kLoss) { Jl[0] *= w; Jl[1] *= w; }
      double *gl = lout + 16L * o0 + row;
      gl[0] = Jl[0];
      gl[nrows] = Jl[1];
      lsum[0] = Jl[0] * r; lsum[1] = Jl[1] * r;
      lsum[2] = Jl[0] * Jl[0]; lsum[3] = Jl[1] * Jl[1];
    }
    if (sw) {
#pragma unroll
      for (int j = 1; j < 7; ++j) {
        const double v = J[j];
        J[j] = J[j + 6];
        J[j + 6] = v;
      }
    }
    double *dst = rows + (long)lr * kRowStride;
    if (scale) {
      const double *sc = scale + slot_cap(P, c);
      const double *st = scale + slot_tag(P, t);
      dst[0] = J[0] * scale[0];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        dst[1 + j] = J[1 + j] * sc[j];
        dst[7 + j] = J[7 + j] * st[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 13; ++j) dst[j] = J[j];
    }
    dst[13] = r;
    if (gout) {
      double *g = gout + 8L * o0 * kJStored + row;
#pragma unroll
      for (int j = 0; j < 13; ++j)
        if (j < 7 || j > 9) g[(long)jrow_col(j) * nrows] = J[j];
      g[(long)jrow_col(13) * nrows] = r;
    }
  }
}

// The per-capture kernels k_linearize (lm_linearize.hip), k_cost and k_backsub
// (lm_step.hip) come in two instances: kChunked = false, the main launch over every capture, which
// takes the captures of at most kObsChunk observations (one wave of rows, the
// code the usual capture runs) and skips the others when there are some;
// true, a second launch over those (DevProblem::chunk_caps), their rows
// through LDS 64 at a time.  The rare large capture's loops then cost the
// usual one no registers or branches.
// kLoss = true: the loaded problem has robust losses (DevProblem::obs_loss_*);
// false is the code without them, instruction for instruction.  k_backsub
// reads the corrected rows k_linearize stored, so its kLoss reaches only the
// fused candidate cost.
// kSized = true: the loaded problem has a tag side other than the default
// (DevProblem::obs_size); false is the code with the constant side,
// instruction for instruction.  The two flags are independent: four instances
// of each form, and a problem of default-size tags launches the two it always
// has.  k_backsub's kSized, like its kLoss, reaches only the candidate cost.
// kDist = true: the problem was loaded under ARSLAM_CAMERA_RADIAL
// (DevProblem::camera_radial); false is the pinhole code, instruction for
// instruction.  Independent of the other two: eight instances of each form,
// and a pinhole problem launches one of the four it always could.
#define ARSLAM_PICK_INSTANCE_D(K, chunked, loss, sized, dist)                               \
  ((sized) ? ((loss) ? K<chunked, true, true, dist> : K<chunked, false, true, dist>)        \
           : ((loss) ? K<chunked, true, false, dist> : K<chunked, false, false, dist>))
#define ARSLAM_PICK_INSTANCE(K, chunked, loss, sized, dist)                                 \
  ((dist) ? ARSLAM_PICK_INSTANCE_D(K, chunked, loss, sized, true)                           \
          : ARSLAM_PICK_INSTANCE_D(K, chunked, loss, sized, false))
// The "estimate the distortion" switch (a DevCamL beside the problem; always
// the radial model): k_linearize_est and k_backsub_est, kernels of their own
// around the same bodies, four instances of each form -- twelve per form in
// all, and the eight the other problems launch keep their names and code.
#define ARSLAM_PICK_INSTANCE_EST(K, chunked, loss, sized)                                   \
  ((sized) ? ((loss) ? K<chunked, true, true> : K<chunked, false, true>)                    \
           : ((loss) ? K<chunked, true, false> : K<chunked, false, false>))
template <bool kChunked>
__device__ __forceinline__ int chunk_capture(const DevProblem &P, int &k) {
  const int c = kChunked ? P.chunk_caps[blockIdx.x] : (int)blockIdx.x;
  k = P.cap_start[c + 1] - P.cap_start[c];
  return (!kChunked && k > kObsChunk) ? -1 : c;   // (-1: the chunked launch's)
}

// The levels of offset < 64 of a block's pairwise tree reduction
// red[t] = op(red[t], red[t + off]) (off = n/2 .. 1), on wave 0 by lane shifts
// instead of an LDS round trip and a block barrier per level: the same pairs
// in the same order, so the same bits.  v: lane t's red[t] after the level of
// offset 64 (n: the elements left, <= 64); the result lands in lane 0.  All of
// wave 0 must be active.
__device__ __forceinline__ double wave_tree_sum(double v, int n) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    if (off < n) v += __shfl_down(v, off, kWave);
  return v;
}
__device__ __forceinline__ double wave_tree_max(double v, int n) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    if (off < n) v = fmax(v, __shfl_down(v, off, kWave));
  return v;
}

// (host) LDS bytes of the rows of maxk observations
size_t lds_rows(int maxk) { return (size_t)8 * maxk * kRowStride * sizeof(double); }

}  // namespace

}  // namespace arslam
