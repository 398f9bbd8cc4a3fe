// lm_cov_host.h -- what the host mirror (host/ar_slam_solver.cpp, plain C++)
// reads of the LM handle's covariance beside the C-ABI; defined in lm_cov_capi.hip.
#pragma once
#include "arslam_lm.h"

namespace arslam {
// The info of the result an _anchored pointer-keyed call keeps on the handle;
// false when none is kept.
bool kept_anchored_cov_info(const arslam_lm *h, arslam_lm_cov_info *info);
}  // namespace arslam
