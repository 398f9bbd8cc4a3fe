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
// (kDist: linearize_min_waves)
template <bool kChunked, bool kLoss, bool kSized, bool kDist>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(linearize_min_waves(kChunked, kSized, kDist), 8))) void k_linearize(DevProblem P, const double *__restrict__ x,
                                                     double *__restrict__ g,
                                                     double *__restrict__ colnorm,
                                                     double *__restrict__ obs_tg,
                                                     double *__restrict__ parts) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int c = kChunked ? P.chunk_caps[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
  const int o0 = P.cap_start[c], k = P.cap_start[c + 1] - o0;
  if (!kChunked && k > kObsChunk) return;   // (the chunked launch's)
  const int nrows = 8 * k;
  // The rows go through LDS in chunks of kObsChunk observations (one wave's
  // 64 rows), so any number of observations per capture fits; every sum runs
  // on over the chunks in the same order as over the whole capture at once
  double *rows = sm;
  double *ocost = rows + (long)8 * kObsChunk * kRowStride;   // [kObsChunk]
  // the running sums carried over the chunks, in LDS (nothing held in
  // registers across the projection): lanes 0..13's per-capture sums, then
  // the active and fixed cost
  double *accs = ocost + kObsChunk;   // [16]
  // (one chunk -- the usual capture -- as its own specialised copy: the loop
  // around the projection cost the single-chunk code spills)
  auto chunk = [&](int q0) __attribute__((always_inline)) {
    const int kc = min(kObsChunk, k - q0), nr = 8 * kc;
    fill_rows<kLoss, kSized, kDist>(P, x, nullptr, c, o0, 8 * q0, nr, nrows, rows, P.jrows, kLoss ? ocost : nullptr);
    __syncthreads();
    // Every sum below is over rows of one product of two LDS columns (ca, cb),
    // picked per lane up front: one code path for the whole wave (a divergent
    // if-chain ran each case's LDS round trips one after another)
    // per observation: cost (r'r), tag gradient (6: F_t'r), tag column norms (6)
    for (int e = lane; e < 13 * kc; e += kWave) {
      const int q = e / 13, it = e % 13;
      const double *rq = rows + (long)q * 8 * kRowStride;
      const int ca = it == 0 ? 13 : it <= 6 ? 6 + it : it, cb = it <= 6 ? 13 : it;
      double s = 0.0;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) s += rq[rr * kRowStride + ca] * rq[rr * kRowStride + cb];
      if (it == 0) {
        if (!kLoss) ocost[q] = 0.5 * s;   // (kLoss: rho / 2, left there by fill_rows)
      }
      else obs_tg[12L * P.obs_tpos[o0 + q0 + q] + (it - 1)] = s;   // (tag-major: k_lin_reduce reads a tag's at once)
    }
    // per capture: capture gradient (6: E'r), capture column norms (6), f gradient, f column norm
    if (lane < 14) {
      const int ca = lane < 6 ? 1 + lane : lane < 12 ? lane - 5 : 0;
      const int cb = lane < 6 ? 13 : lane < 12 ? lane - 5 : lane == 12 ? 13 : 0;
      double ps = q0 ? accs[lane] : 0.0;
#pragma unroll 8
      for (int r = 0; r < nr; ++r) ps += row_prod(rows + (long)r * kRowStride, ca, cb);
      accs[lane] = ps;
    }
    __syncthreads();
    if (lane == 0) {
      double act = q0 ? accs[14] : 0.0, fix = q0 ? accs[15] : 0.0;
      for (int q = 0; q < kc; ++q) {
        if (P.obs_active[o0 + q0 + q]) act += ocost[q]; else fix += ocost[q];
      }
      accs[14] = act;
      accs[15] = fix;
    }
  };
  if (!kChunked) {   // (at most one chunk)
    chunk(0);
  } else {
    for (int q0 = 0; q0 < k; q0 += kObsChunk) {
      if (q0) __syncthreads();   // the previous chunk's LDS reads are done
      chunk(q0);
    }
  }
  if (lane < 14) {
    const double ps = k ? accs[lane] : 0.0;
    if (lane < 12) {
      const long slot = slot_cap(P, c) + (lane % 6);
      const double v = P.slot_free[slot] ? ps : 0.0;
      if (lane < 6) g[slot] = v; else colnorm[slot] = v;
    } else if (lane == 12) {
      parts[(long)P_GF * P.nc + c] = ps;
    } else {
      parts[(long)P_CF * P.nc + c] = ps;
    }
  }
  if (lane == 0) {
    parts[(long)P_COST * P.nc + c] = k ? accs[14] : 0.0;
    parts[(long)P_FIXED * P.nc + c] = k ? accs[15] : 0.0;
  }
}

}  // namespace

void launch_linearize(const DevProblem &P, const double *x, double *g, double *colnorm,
                      double *obs_tg, double *parts, hipStream_t s) {
  if (P.nc == 0) return;
  const size_t lds = lds_rows(kObsChunk) + sizeof(double) * (kObsChunk + 16);
  // (the instance per loaded problem: kLoss iff it has robust losses, kSized
  // iff some tag's side is not the default, kDist iff loaded under the radial model)
  const bool loss = P.obs_loss_kind != nullptr, sized = P.obs_size != nullptr, dist = P.camera_radial != 0;
  hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE(k_linearize, false, loss, sized, dist), dim3(P.nc), dim3(kWave), lds, s, P,
                     x, g, colnorm, obs_tg, parts);
  if (P.n_chunk_caps)
    hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE(k_linearize, true, loss, sized, dist), dim3(P.n_chunk_caps), dim3(kWave),
                       lds, s, P, x, g, colnorm, obs_tg, parts);
}

}  // namespace arslam
