// lm_linearize.hip -- the linearization of the LM step (fp64, gfx950).
//
// k_linearize, one wavefront per capture: its lanes evaluate the capture's
// residual rows and analytic Jacobian into LDS (fill_rows: lane l of a 64-row
// chunk owns row l) and store the unscaled rows to DevProblem::jrows, which
// k_schur and k_backsub reload at the same point.  From LDS the wave forms
// the per-observation tag gradient and column-norm sums (obs_tg, one lane per
// (observation, entry)), the capture's own gradient and column norms (lanes
// 0..11), the camera-f partials (lanes 12, 13) and the active / fixed cost
// (lane 0).  lm_reduce.hip sums what it leaves per capture and per
// observation.
//
// Every sum is fixed-order (no atomics): over an observation's 8 rows, then
// over the capture's rows chunk by chunk in row order.
//
// k_linearize_est, the same body (lm_linearize_body.h) for a problem whose
// l1, l2 are estimated: it also stores the rows' two l columns and leaves the
// capture's l gradient and column-norm partials.
#include "lm_launch.h"
#include "lm_rows.h"

namespace arslam {

namespace {

// rr[ca] * rr[cb], rounded before it is added (no FMA contraction: the
// per-capture sums of k_linearize have always rounded product and sum
// separately, the per-observation ones use FMAs; kept as they were)
__device__ __forceinline__ double row_prod(const double *rr, int ca, int cb) {
#pragma clang fp contract(off)
  return rr[ca] * rr[cb];
}

// The least waves per SIMD k_linearize asks the register allocator to keep.
// The pinhole instances: 4, and 2 for the sized chunked ones (the comments at
// the kernel).  The radial ones hold d, d' and the two products of P on top of
// the pinhole row: an instance that would spill at its pinhole twin's bound
// asks for fewer waves instead of scratch (profiles/distortion/resource_usage.txt).
constexpr int linearize_min_waves(bool chunked, bool sized, bool dist) {
  return (chunked && (sized || dist)) ? 2 : 4;
}

// (4 waves per SIMD instead of the 3 its 143 VGPRs allow: a 28-byte spill,
// 84 -> 71 us on cfg3; 5 waves spills 148 bytes and is slower)
// (those figures are the compiler's of the time.  Today's gives, under the
// same attribute, 96 VGPRs and no scratch for <false, false> -- 5 waves --
// and 128 VGPRs and 12 bytes for <true, false>; with kLoss 98 / 0 and
// 128 / 88, 4 waves: DESIGN §2b, profiles/loss/resource_usage.txt)
// Linearize at x: per-observation tag gradient/column norms, per-capture
// gradient/column norms, cost and camera partials.  Unscaled Jacobian (with
// kLoss: corrected by sqrt(rho') per observation).
// (kSized: the same attribute for the one-chunk instances, 96 / 98 VGPRs as
// without; the chunked ones ask for 2 waves instead of 4 and so take the
// registers the others spill for: no scratch, profiles/tag_size/resource_usage.txt)
// (kDist: linearize_min_waves; the body: lm_linearize_body.h)
template <bool kChunked, bool kLoss, bool kSized, bool kDist>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(linearize_min_waves(kChunked, kSized, kDist), 8))) void k_linearize(DevProblem P, const double *__restrict__ x,
                                                     double *__restrict__ g,
                                                     double *__restrict__ colnorm,
                                                     double *__restrict__ obs_tg,
                                                     double *__restrict__ parts) {
  constexpr int kMode = kDist ? 1 : 0;
  constexpr double *lparts = nullptr, *jrows_l = nullptr;
#include "lm_linearize_body.h"
}

// The instance of a problem whose l1, l2 are estimated (DevCamL): the radial
// rows, their two l columns into jrows_l and the l partials into lparts.  (the
// radial instances' register bound)
template <bool kChunked, bool kLoss, bool kSized>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(linearize_min_waves(kChunked, kSized, true), 8))) void k_linearize_est(DevProblem P, const double *__restrict__ x,
                                                     double *__restrict__ g,
                                                     double *__restrict__ colnorm,
                                                     double *__restrict__ obs_tg,
                                                     double *__restrict__ parts,
                                                     double *__restrict__ lparts,
                                                     double *__restrict__ jrows_l) {
  constexpr int kMode = 2;
#include "lm_linearize_body.h"
}

}  // namespace

void launch_linearize(const DevProblem &P, const double *x, double *g, double *colnorm,
                      double *obs_tg, double *parts, hipStream_t s, const DevCamL *cl) {
  if (P.nc == 0) return;
  const size_t lds = lds_rows(kObsChunk) + sizeof(double) * (kObsChunk + 16);
  // (the instance per loaded problem: kLoss iff it has robust losses, kSized
  // iff some tag's side is not the default, kDist iff loaded under the radial model)
  const bool loss = P.obs_loss_kind != nullptr, sized = P.obs_size != nullptr, dist = P.camera_radial != 0;
  if (cl) {   // l1, l2 estimated: the instances that also leave the l columns and partials
    hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE_EST(k_linearize_est, false, loss, sized), dim3(P.nc), dim3(kWave), lds, s, P,
                       x, g, colnorm, obs_tg, parts, cl->lparts, cl->jrows_l);
    if (P.n_chunk_caps)
      hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE_EST(k_linearize_est, true, loss, sized), dim3(P.n_chunk_caps),
                         dim3(kWave), lds, s, P, x, g, colnorm, obs_tg, parts, cl->lparts, cl->jrows_l);
    return;
  }
  hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE(k_linearize, false, loss, sized, dist), dim3(P.nc), dim3(kWave), lds, s, P,
                     x, g, colnorm, obs_tg, parts);
  if (P.n_chunk_caps)
    hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE(k_linearize, true, loss, sized, dist), dim3(P.n_chunk_caps), dim3(kWave),
                       lds, s, P, x, g, colnorm, obs_tg, parts);
}

}  // namespace arslam
