// loss.h -- the robust loss functions of a residual block (Ceres 2.0
// loss_function.cc): rho(s) and rho'(s) of s = |r|^2, by kind and scale a.
// Shared by the per-capture kernels (lm_rows.h: the corrected rows
// sqrt(rho') r, sqrt(rho') J; lm_step.hip: the cost rho / 2), the debug entry
// arslam_debug_residual_jacobian_loss and the host's argument checks.
//
// Every loss here has rho'' <= 0, so Ceres' Corrector (corrector.cc) always
// takes its alpha = 0 branch: the rows are scaled by sqrt(rho') and nothing
// else.  A loss with rho'' > 0 (Tolerant) needs the full corrector.
#pragma once
#include <cfloat>
#include <cmath>

#include "arslam_lm.h"

#if defined(__HIPCC__)
#define ARSLAM_LOSS_HD __host__ __device__
#else
#define ARSLAM_LOSS_HD
#endif

namespace arslam {

// kinds [0, kLossKinds) are implemented (the enum of arslam_lm.h; later kinds append)
constexpr int kLossKinds = 4;

ARSLAM_LOSS_HD inline bool loss_valid(int kind, double a) {
  if (kind < 0 || kind >= kLossKinds) return false;
  return kind == ARSLAM_LOSS_NONE || (a > 0.0 && a <= DBL_MAX);   // (finite and > 0; NaN fails both)
}

// rho(s) and rho'(s); b = a^2
ARSLAM_LOSS_HD inline void loss_eval(int kind, double a, double s, double *rho, double *rho1) {
  const double b = a * a;
  switch (kind) {
    case ARSLAM_LOSS_HUBER:
      if (s > b) {
        const double r = sqrt(s);
        *rho = 2.0 * a * r - b;
        *rho1 = fmax(DBL_MIN, a / r);
      } else {
        *rho = s;
        *rho1 = 1.0;
      }
      break;
    case ARSLAM_LOSS_SOFT_L_ONE: {
      const double sum = 1.0 + s / b;
      const double tmp = sqrt(sum);
      *rho = 2.0 * b * (tmp - 1.0);
      *rho1 = fmax(DBL_MIN, 1.0 / tmp);
      break;
    }
    case ARSLAM_LOSS_CAUCHY: {
      const double sum = 1.0 + s / b;
      *rho = b * log(sum);
      *rho1 = fmax(DBL_MIN, 1.0 / sum);
      break;
    }
    default:   // ARSLAM_LOSS_NONE
      *rho = s;
      *rho1 = 1.0;
      break;
  }
}

}  // namespace arslam
