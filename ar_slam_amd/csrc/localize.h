// localize.h -- the seam between the localizer's kernels (localize.hip) and its
// handle and C-ABI (localize_capi.hip): the kernels' argument structs and their
// launchers.
#pragma once
#include <hip/hip_runtime.h>

#include "arslam_localize.h"

namespace arslam {

// k_localize's arguments: the loaded batch, the options and the resident losses
struct LocParams {
  int nq, nt;
  const double *cam;           // [3]
  const double *tag;           // [nt*6]
  const unsigned char *tim;    // [nt] or null
  const int *qs;               // [nq+1]
  const int *ot;               // [nb]
  const double *corners;       // [nb*8]
  const double *pose_in;       // [nq*6]
  double *pose_out;            // [nq*6]
  arslam_localize_result *res; // [nq]
  const double *aw;            // [nt*4][4] world points of the (constant) tags' corners
  int init_from_map, max_k;
  int max_iters, max_invalid, jacobi;
  // 1: ARSLAM_CAMERA_RADIAL -- the launchers pick the kDist instances, which
  // read l1, l2 from cam[1], cam[2]; no kernel reads the flag.  (In the four
  // bytes that padded jacobi up to ftol: no field's kernel-argument offset moves.)
  int dist;
  double ftol, gtol, ptol, r0, rmax, rmin, min_rel, dmin, dmax;
  // per-observation robust loss (ARSLAM_LOSS_*, scale), read by the kLoss
  // instances only; null when no observation of the batch has one
  const unsigned char *lk;     // [nb]
  const double *la;            // [nb]
  // the map tags' sides in metres; null when every tag has the default side
  // (last in the struct: no other field's kernel-argument offset moves)
  const double *tsize;         // [nt]
};

// k_localize_cov's: k_localize's arguments (the batch, the last solve's poses, results, losses
// and aw) and the three outputs.
struct LocCovParams {
  LocParams p;
  double *cov;       // [nq*36]
  int *cov_status;   // [nq]
  double *min_pivot; // [nq]
};

// k_tag_corners (p.aw from the map) and the k_localize instance p.max_k and p.lk choose
void launch_localize(const LocParams &p, hipStream_t s);
// k_localize_cov on what the last solve left on the device
void launch_localize_cov(const LocCovParams &cp, hipStream_t s);
// k_localize_terms at p.pose_out / p.res: sq_out, w_out [n_obs] (device)
void launch_localize_terms(const LocParams &p, double *sq_out, double *w_out, hipStream_t s);

}  // namespace arslam
