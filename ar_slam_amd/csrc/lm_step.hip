// lm_step.hip -- the candidate of the LM step: back-substitution, the f-side
// update and the cost (fp64, gfx950).
//
// k_backsub, one wavefront per capture: the wave reloads the rows k_linearize
// stored (load_rows_q: lane l owns row l of a 64-row chunk, and forms the
// row's reduced-side product F_row . y_F), solves the capture's 6x6 system for
// its step, writes the candidate's capture slots and the capture's share of
// the model cost change, and, fused, the candidate's cost (capture_cost, which
// k_cost runs alone: lane l re-evaluates residual row l at the candidate).
// k_update_f, one thread per reduced row / f-side slot, writes the candidate's
// camera and tag slots from the reduced solution.
//
// k_backsub_est, the same body (lm_backsub_body.h) for a problem whose l1, l2
// are estimated: F_row . y_F takes in the rows' two l columns.
//
// Every sum is fixed-order (no atomics): each lane's sums run over the rows in
// row order, the costs over the observations in observation order; the
// per-capture partials are reduced by lm_reduce.hip.
#include "lm_launch.h"
#include "lm_rows.h"

#include <algorithm>

namespace arslam {

namespace {

// LDS rows [row0, row0 + nr) of capture c (nrows rows in all) from the copy
// fill_rows stored at the same point, Jacobi-scaled, and each row's
// reduced-side product
//   qv[row] = F_row . y_F = J_f y_f + J_t . y_F[tag rows]
// formed from the row the lane just scaled (its tag row and y_F loads go out
// beside the Jacobian loads instead of after a barrier).
// kEst (l1, l2 estimated; jrows_l: DevCamL's): plus the two l columns' terms,
// J_l1 s_1 yl1 + J_l2 s_2 yl2 (yl: y of reduced rows cam_row + 1, cam_row + 2).
template <bool kEst = false>
__device__ __forceinline__ void load_rows_q(const DevProblem &P, const double *scale, const double *yF, double yf, int c, int o0,
                            int row0, int nr, int nrows, double *rows, double *qv, double yl1 = 0.0,
                            double yl2 = 0.0, const double *jrows_l = nullptr) {
  const double *sc = scale + slot_cap(P, c);
  for (int lr = threadIdx.x; lr < nr; lr += kWave) {
    const int row = row0 + lr;
    const double *g = P.jrows + 8L * o0 * kJStored + row;
    const int t = P.obs_tag[o0 + (row >> 3)];
    const int tr = P.tag_row[t];
    double u[kJStored], v[14];
#pragma unroll
    for (int j = 0; j < kJStored; ++j) u[j] = g[(long)j * nrows];
#pragma unroll
    for (int j = 0; j < 14; ++j) v[j] = u[jrow_col(j)];
    const double *st = scale + slot_tag(P, t);
    double yt[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) yt[j] = tr >= 0 ? yF[tr + j] : 0.0;
    double *dst = rows + (long)lr * kRowStride;
    double d[14];
    d[0] = v[0] * scale[0];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      d[1 + j] = v[1 + j] * sc[j];
      d[7 + j] = v[7 + j] * st[j];
    }
    d[13] = v[13];
#pragma unroll
    for (int j = 0; j < 14; ++j) dst[j] = d[j];
    double q = d[0] * yf;
    if (tr >= 0) {
#pragma unroll
      for (int j = 0; j < 6; ++j) q += d[7 + j] * yt[j];
    }
    if (kEst) {
      const double *gl = jrows_l + 16L * o0 + row;
      q += (gl[0] * scale[1]) * yl1 + (gl[nrows] * scale[2]) * yl2;
    }
    qv[lr] = q;
  }
}

// (a,b) of the e-th entry of the upper triangle of a 6x6 matrix, row-major
__device__ __forceinline__ void upper6(int e, int &a, int &b) {
  a = 0;
  int rem = e;
  while (rem >= 6 - a) { rem -= 6 - a; ++a; }
  b = a + rem;
}

// 6x6 SPD inverse by LLT + two triangular solves against I (Ceres'
// InvertPSDMatrix<full rank>); single lane.
__device__ void inv6(const double *U, double *Ui) {
  double L[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) L[i] = U[i];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double xj = L[6 * j + j];
#pragma unroll
    for (int p = 0; p < j; ++p) xj -= L[6 * j + p] * L[6 * j + p];
    const double d = sqrt(xj);
    L[6 * j + j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = L[6 * i + j];
#pragma unroll
      for (int p = 0; p < j; ++p) v -= L[6 * i + p] * L[6 * j + p];
      L[6 * i + j] = v / d;
    }
  }
#pragma unroll
  for (int col = 0; col < 6; ++col) {
    double e[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double v = (i == col) ? 1.0 : 0.0;
#pragma unroll
      for (int p = 0; p < i; ++p) v -= L[6 * i + p] * e[p];
      e[i] = v / L[6 * i + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double v = e[i];
#pragma unroll
      for (int p = i + 1; p < 6; ++p) v -= L[6 * p + i] * e[p];
      e[i] = v / L[6 * i + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) Ui[6 * i + col] = e[i];
  }
}

// Cost at x (candidate evaluation) of capture c: active / fixed cost,
// finiteness.  cap: the capture's 6 parameters (x's slot, or the candidate
// k_backsub just formed, held in LDS); camera and tags from x.
// (kChunked: a capture of more than kObsChunk observations, its rows 64 at a
// time; else at most one wave of rows)
template <bool kChunked, bool kLoss, bool kSized, bool kDist>
__device__ __forceinline__ void capture_cost(const DevProblem &P, const double *__restrict__ x, const double *cap,
                                             int c, double *__restrict__ parts) {
  __shared__ double sq[kWave];
  __shared__ double ocost[kObsChunk];   // (per 64-row chunk; summed in observation order)
  const int lane = threadIdx.x;
  const int o0 = P.cap_start[c], k = P.cap_start[c + 1] - o0;
  const int nrows = 8 * k;
  const double *cam = x;
  const AngleAxis ac = aa_prepare(cap + 3);
  double bad = 0.0, act = 0.0, fix = 0.0;
  for (int base = 0; base < (kChunked ? nrows : 1); base += kWave) {
    const int row = base + lane;
    double r2 = 0.0;
    if (row < nrows) {
      const int q = row >> 3, corner = (row >> 1) & 3, comp = row & 1;
      const int obs = o0 + q;
      const double *tag = x + slot_tag(P, P.obs_tag[obs]);
      const AngleAxis at = aa_prepare(tag + 3);
      const double obsv = P.corners[8L * obs + 2 * corner + comp];
      const bool sw = group_swapped(P, c);   // tag e-block: the capture is the f-block
      const double half = kSized ? 0.5 * P.obs_size[obs] : kArucoHalf;
      // (kDist: the radial model's l1, l2 from camera slots 1, 2)
      const double r = kDist ? residual_row<true>(sw ? at : ac, sw ? tag : cap, sw ? ac : at, sw ? cap : tag, cam[0],
                                                  half, corner, comp, obsv, nullptr, nullptr, cam[1], cam[2])
                             : residual_row(sw ? at : ac, sw ? tag : cap, sw ? ac : at, sw ? cap : tag, cam[0], half,
                                            corner, comp, obsv, nullptr, nullptr);
      if (!isfinite(r)) bad = 1.0;
      r2 = r * r;
    }
    sq[lane] = r2;
    __syncthreads();
    if (lane < 8 && base / 8 + lane < k) {
      double s = 0.0;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) s += sq[8 * lane + rr];
      if (kLoss) {   // the cost is rho(s) / 2
        const int obs = o0 + base / 8 + lane;
        double rho1;
        loss_eval(P.obs_loss_kind[obs], P.obs_loss_a[obs], s, &s, &rho1);
      }
      ocost[lane] = 0.5 * s;
    }
    __syncthreads();
    if (kChunked && lane == 0)
      for (int q = base / 8; q < min(k, base / 8 + kObsChunk); ++q) {
        if (P.obs_active[o0 + q]) act += ocost[q - base / 8]; else fix += ocost[q - base / 8];
      }
  }
  if (!kChunked && lane == 0)
    for (int q = 0; q < k; ++q) {
      if (P.obs_active[o0 + q]) act += ocost[q]; else fix += ocost[q];
    }
  bad = wave_max(bad);
  if (lane == 0) {
    parts[(long)P_COST * P.nc + c] = act;
    parts[(long)P_FIXED * P.nc + c] = fix;
    parts[(long)P_CBAD * P.nc + c] = bad;
  }
}

template <bool kChunked, bool kLoss, bool kSized, bool kDist>
__global__ __launch_bounds__(kWave) void k_cost(DevProblem P, const double *__restrict__ x,
                                                double *__restrict__ parts) {
  int k;
  const int c = chunk_capture<kChunked>(P, k);
  if (c < 0) return;
  capture_cost<kChunked, kLoss, kSized, kDist>(P, x, x + slot_cap(P, c), c, parts);
}

// Back substitution for capture c, candidate update of its slots and its
// share of the model cost change.  (the body: lm_backsub_body.h)
template <bool kChunked, bool kLoss, bool kSized, bool kDist>
__global__ __launch_bounds__(kWave) void k_backsub(DevProblem P, const double *__restrict__ x,
                                                   const double *__restrict__ scale,
                                                   const double *__restrict__ diag, double radius,
                                                   const double *__restrict__ yF,
                                                   double *__restrict__ xc,
                                                   double *__restrict__ parts, int reuse_ui, int with_cost) {
  constexpr bool kEst = false;
  constexpr const double *jrows_l = nullptr;
#include "lm_backsub_body.h"
}

// The instance of a problem whose l1, l2 are estimated (DevCamL::jrows_l):
// the rows' products with the reduced solution include the two l columns; the
// candidate's cost is the radial model's, at the candidate's l1, l2.
template <bool kChunked, bool kLoss, bool kSized>
__global__ __launch_bounds__(kWave) void k_backsub_est(DevProblem P, const double *__restrict__ x,
                                                       const double *__restrict__ scale,
                                                       const double *__restrict__ diag, double radius,
                                                       const double *__restrict__ yF,
                                                       double *__restrict__ xc,
                                                       double *__restrict__ parts, int reuse_ui, int with_cost,
                                                       const double *__restrict__ jrows_l) {
  constexpr bool kEst = true, kDist = true;
#include "lm_backsub_body.h"
}

// Candidate update of the tag and camera slots from the reduced solution
// (every f-side slot of xc is written, so xc needs no copy of x first:
// k_backsub writes every capture slot).
__global__ __launch_bounds__(256) void k_update_f(DevProblem P, const double *__restrict__ x,
                                                  const double *__restrict__ scale,
                                                  const double *__restrict__ yF,
                                                  double *__restrict__ xc,
                                                  double *__restrict__ fparts) {
  __shared__ double red[2][256];
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double st = 0.0, bad = 0.0;
  const long slot = i < P.nR ? P.row_slot[i] : -1;
  if (slot >= 0) {   // reduced row i
    const double yv = yF[i];
    const double xo = x[slot];
    const double xn = xo + (-yv * scale[slot]);
    xc[slot] = xn;
    // (several ranks: each slot's step counted on the rank holding it)
    if (P.slot_free[slot] && (!P.f_own || P.f_own[slot])) st = (xo - xn) * (xo - xn);
    bad = isfinite(yv) ? 0.0 : 1.0;
  }
  if (i < P.nf && P.fslot_row[i] < 0) {   // f-side slot i outside the reduced system: unchanged
    const long fs = i < 3 ? i : 3 + 6L * P.nc + (i - 3);
    xc[fs] = x[fs];
  }
  if ((long)blockIdx.x * blockDim.x >= P.nR) return;   // (partials: one per 256 reduced rows)
  red[0][threadIdx.x] = st;
  red[1][threadIdx.x] = bad;
  __syncthreads();
  for (int off = 128; off >= kWave; off >>= 1) {
    if (threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] = fmax(red[1][threadIdx.x], red[1][threadIdx.x + off]);
    }
    __syncthreads();
  }
  if (threadIdx.x < kWave) {
    const double s0 = wave_tree_sum(red[0][threadIdx.x], kWave);
    const double s1 = wave_tree_max(red[1][threadIdx.x], kWave);
    if (threadIdx.x == 0) {
      fparts[2L * blockIdx.x] = s0;
      fparts[2L * blockIdx.x + 1] = s1;
    }
  }
}

}  // namespace

void launch_backsub(const DevProblem &P, const double *x, const double *scale, const double *diag,
                    double radius, const double *yF, double *xc, double *parts, hipStream_t s,
                    bool reuse_ui, bool with_cost, const DevCamL *cl) {
  if (P.nc == 0) return;
  const size_t lds = lds_rows(kObsChunk) + sizeof(double) * (8L * kObsChunk + 36 + 36 + 16);
  const bool loss = P.obs_loss_kind != nullptr, sized = P.obs_size != nullptr, dist = P.camera_radial != 0;
  if (cl) {   // l1, l2 estimated
    hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE_EST(k_backsub_est, false, loss, sized), dim3(P.nc), dim3(kWave), lds, s, P,
                       x, scale, diag, radius, yF, xc, parts, reuse_ui ? 1 : 0, with_cost ? 1 : 0, cl->jrows_l);
    if (P.n_chunk_caps)
      hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE_EST(k_backsub_est, true, loss, sized), dim3(P.n_chunk_caps), dim3(kWave),
                         lds, s, P, x, scale, diag, radius, yF, xc, parts, reuse_ui ? 1 : 0, with_cost ? 1 : 0,
                         cl->jrows_l);
    return;
  }
  hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE(k_backsub, false, loss, sized, dist), dim3(P.nc), dim3(kWave), lds, s, P, x,
                     scale, diag, radius, yF, xc, parts, reuse_ui ? 1 : 0, with_cost ? 1 : 0);
  if (P.n_chunk_caps)
    hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE(k_backsub, true, loss, sized, dist), dim3(P.n_chunk_caps), dim3(kWave), lds, s,
                       P, x, scale, diag, radius, yF, xc, parts, reuse_ui ? 1 : 0, with_cost ? 1 : 0);
}

void launch_update_f(const DevProblem &P, const double *x, const double *scale, const double *yF,
                     double *xc, double *fparts, hipStream_t s) {
  const long n = std::max<long>(P.nR, P.nf);
  if (n == 0) return;
  hipLaunchKernelGGL(k_update_f, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, x, scale, yF, xc, fparts);
}

void launch_cost(const DevProblem &P, const double *x, double *parts, hipStream_t s) {
  if (P.nc == 0) return;
  const bool loss = P.obs_loss_kind != nullptr, sized = P.obs_size != nullptr, dist = P.camera_radial != 0;
  hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE(k_cost, false, loss, sized, dist), dim3(P.nc), dim3(kWave), 0, s, P, x, parts);
  if (P.n_chunk_caps)
    hipLaunchKernelGGL(ARSLAM_PICK_INSTANCE(k_cost, true, loss, sized, dist), dim3(P.n_chunk_caps), dim3(kWave), 0, s, P, x,
                       parts);
}

}  // namespace arslam
