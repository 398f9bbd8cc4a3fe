// debug_rows.hip -- component entry points (include/arslam_lm_debug.h) over the
// per-row device functions: the residual and Jacobian rows, the same rows under
// a robust loss, and AngleAxisRotatePoint, each run alone so the parity tests
// can pin it to the oracle.
#include "hip_host.h"
#include "lm_rows.h"
#include "loss.h"
#include "projection.h"
#include "arslam_lm.h"
#include "arslam_lm_debug.h"

#include <vector>

namespace arslam {
namespace {

// one thread per (observation, row): residual and 15-column Jacobian row
// (kSized: of a tag of side size[o]; else of the default side, size unused;
// kDist: under the radial camera model, l1 and l2 from cam, else the pinhole)
template <bool kSized, bool kDist = false>
__global__ void k_debug_rj(int n, const double *__restrict__ cam, const double *__restrict__ cap,
                           const double *__restrict__ tag, const double *__restrict__ corners,
                           const double *__restrict__ size, double *__restrict__ r, double *__restrict__ J) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 8L * n) return;
  const long o = e / 8;
  const int row = (int)(e % 8), corner = row >> 1, comp = row & 1;
  double j13[13];
  r[e] = residual_jacobian_row<kDist>(cam + 3 * o, cap + 6 * o, tag + 6 * o, kSized ? 0.5 * size[o] : kArucoHalf,
                                      corner, comp, corners[8 * o + row], j13);
  double *out = J + e * 15;
  out[0] = j13[0];
  out[1] = 0.0;
  out[2] = 0.0;
  for (int j = 0; j < 12; ++j) out[3 + j] = j13[1 + j];
}

// one thread per (observation, row): the radial model's residual and the row's
// two l columns (residual_jacobian_row's Jl, as fill_rows<.., 2> takes them)
template <bool kSized>
__global__ void k_debug_rj_l(int n, const double *__restrict__ cam, const double *__restrict__ cap,
                             const double *__restrict__ tag, const double *__restrict__ corners,
                             const double *__restrict__ size, double *__restrict__ r, double *__restrict__ Jl) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 8L * n) return;
  const long o = e / 8;
  const int row = (int)(e % 8), corner = row >> 1, comp = row & 1;
  double j13[13], jl[2];
  r[e] = residual_jacobian_row<true>(cam + 3 * o, cap + 6 * o, tag + 6 * o, kSized ? 0.5 * size[o] : kArucoHalf,
                                     corner, comp, corners[8 * o + row], j13, jl);
  Jl[2 * e] = jl[0];
  Jl[2 * e + 1] = jl[1];
}

// the same rows corrected for each observation's loss (robustify_row, as
// fill_rows<true> forms them) and rho(s) per observation; 8 n is a multiple of
// 8, so an observation's 8 lanes are active together
__global__ void k_debug_rj_loss(int n, const double *__restrict__ cam, const double *__restrict__ cap,
                                const double *__restrict__ tag, const double *__restrict__ corners,
                                const unsigned char *__restrict__ kind, const double *__restrict__ a,
                                double *__restrict__ r, double *__restrict__ J, double *__restrict__ rho) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 8L * n) return;
  const long o = e / 8;
  const int row = (int)(e % 8), corner = row >> 1, comp = row & 1;
  double j13[13];
  double rv = residual_jacobian_row(cam + 3 * o, cap + 6 * o, tag + 6 * o, kArucoHalf, corner, comp,
                                    corners[8 * o + row], j13);
  const double rh = robustify_row(kind[o], a[o], rv, j13);
  r[e] = rv;
  if (row == 0) rho[o] = rh;
  double *out = J + e * 15;
  out[0] = j13[0];
  out[1] = 0.0;
  out[2] = 0.0;
  for (int j = 0; j < 12; ++j) out[3 + j] = j13[1 + j];
}

// AngleAxisRotatePoint of n (w, p) pairs with the branch each one took
// (1: theta^2 > DBL_EPSILON, Rodrigues; 0: x + w x p) -- parity of the
// small-angle branch, ar_slam_util.cpp:145,155.
__global__ void k_debug_aa(int n, const double *__restrict__ w, const double *__restrict__ p,
                           double *__restrict__ out, int *__restrict__ branch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AngleAxis a = aa_prepare(w + 3L * i);
  aa_rotate(a, p + 3L * i, out + 3L * i);
  branch[i] = a.big ? 1 : 0;
}

// n observations' inputs as one device array: cam [3] | cap [6] | tag [6] | corners [8] (| a [1])
void upload_rows(DevBuf<double> &d, int n, const double *cam, const double *cap, const double *tag,
                 const double *corners, const double *a) {
  std::vector<double> h;
  h.reserve((size_t)n * 24);
  h.insert(h.end(), cam, cam + 3L * n);
  h.insert(h.end(), cap, cap + 6L * n);
  h.insert(h.end(), tag, tag + 6L * n);
  h.insert(h.end(), corners, corners + 8L * n);
  if (a) h.insert(h.end(), a, a + n);
  d.alloc(h.size());
  HIP_CHECK(hipMemcpy(d.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
}

template <class T>
void download(T *host, const T *dev, size_t count) {
  HIP_CHECK(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
}

dim3 blocks_of_128(long threads) { return dim3((unsigned)((threads + 127) / 128)); }

}  // namespace
}  // namespace arslam

using arslam::DevBuf;

// the body of the three row entries (size: null = every tag of the default side)
static int debug_rows(int n, const double *cam, const double *cap, const double *tag, const double *corners,
                      const double *size, double *r, double *J, int model = ARSLAM_CAMERA_PINHOLE) {
  if (n < 0 || (n && (!cam || !cap || !tag || !corners || !r || !J))) return ARSLAM_E_INVALID_ARG;
  for (int i = 0; size && i < n; ++i)
    if (!arslam::tag_size_valid(size[i])) return ARSLAM_E_INVALID_ARG;
  if (n == 0) return ARSLAM_OK;
  return arslam::api_guarded([&] {
    DevBuf<double> d_in, d_out;   // d_in: ... (| size [n]); d_out: r [8 n] | J [120 n]
    arslam::upload_rows(d_in, n, cam, cap, tag, corners, size);
    d_out.alloc(128L * n);
    double *d_r = d_out.p, *d_J = d_r + 8L * n;
    const double *d_size = size ? d_in.p + 23L * n : nullptr;
    auto kernel = model == ARSLAM_CAMERA_RADIAL
                      ? (size ? arslam::k_debug_rj<true, true> : arslam::k_debug_rj<false, true>)
                      : (size ? arslam::k_debug_rj<true> : arslam::k_debug_rj<false>);
    hipLaunchKernelGGL(kernel, arslam::blocks_of_128(8L * n), dim3(128), 0, 0, n, d_in.p, d_in.p + 3L * n,
                       d_in.p + 9L * n, d_in.p + 15L * n, d_size, d_r, d_J);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    arslam::download(r, d_r, 8L * n);
    arslam::download(J, d_J, 120L * n);
  });
}

extern "C" int arslam_debug_residual_jacobian(int n, const double *cam, const double *cap,
                                              const double *tag, const double *corners, double *r,
                                              double *J) {
  return debug_rows(n, cam, cap, tag, corners, nullptr, r, J);
}

extern "C" int arslam_debug_residual_jacobian_sized(int n, const double *cam, const double *cap,
                                                    const double *tag, const double *corners,
                                                    const double *size, double *r, double *J) {
  if (n > 0 && !size) return ARSLAM_E_INVALID_ARG;
  return debug_rows(n, cam, cap, tag, corners, size, r, J);
}

extern "C" int arslam_debug_residual_jacobian_model(int n, int model, const double *cam, const double *cap,
                                                    const double *tag, const double *corners,
                                                    const double *size, double *r, double *J) {
  if (!ARSLAM_CAMERA_MODEL_VALID(model)) return ARSLAM_E_INVALID_ARG;
  return debug_rows(n, cam, cap, tag, corners, size, r, J, model);
}

extern "C" int arslam_debug_residual_jacobian_distortion(int n, const double *cam, const double *cap,
                                                         const double *tag, const double *corners,
                                                         const double *size, double *r, double *Jl) {
  if (n < 0 || (n && (!cam || !cap || !tag || !corners || !r || !Jl))) return ARSLAM_E_INVALID_ARG;
  for (int i = 0; size && i < n; ++i)
    if (!arslam::tag_size_valid(size[i])) return ARSLAM_E_INVALID_ARG;
  if (n == 0) return ARSLAM_OK;
  return arslam::api_guarded([&] {
    DevBuf<double> d_in, d_out;   // d_out: r [8 n] | Jl [16 n]
    arslam::upload_rows(d_in, n, cam, cap, tag, corners, size);
    d_out.alloc(24L * n);
    double *d_r = d_out.p, *d_J = d_r + 8L * n;
    const double *d_size = size ? d_in.p + 23L * n : nullptr;
    auto kernel = size ? arslam::k_debug_rj_l<true> : arslam::k_debug_rj_l<false>;
    hipLaunchKernelGGL(kernel, arslam::blocks_of_128(8L * n), dim3(128), 0, 0, n, d_in.p, d_in.p + 3L * n,
                       d_in.p + 9L * n, d_in.p + 15L * n, d_size, d_r, d_J);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    arslam::download(r, d_r, 8L * n);
    arslam::download(Jl, d_J, 16L * n);
  });
}

extern "C" int arslam_debug_residual_jacobian_loss(int n, const double *cam, const double *cap,
                                                   const double *tag, const double *corners,
                                                   const unsigned char *kind, const double *a, double *r,
                                                   double *J, double *rho) {
  if (n < 0 || (n && (!cam || !cap || !tag || !corners || !kind || !a || !r || !J || !rho))) return ARSLAM_E_INVALID_ARG;
  for (int i = 0; i < n; ++i)
    if (!arslam::loss_valid(kind[i], a[i])) return ARSLAM_E_INVALID_ARG;
  if (n == 0) return ARSLAM_OK;
  return arslam::api_guarded([&] {
    DevBuf<double> d_in, d_out;   // d_out: r [8 n] | J [120 n] | rho [n]
    DevBuf<unsigned char> d_k;
    arslam::upload_rows(d_in, n, cam, cap, tag, corners, a);
    d_k.alloc(n);
    HIP_CHECK(hipMemcpy(d_k.p, kind, (size_t)n, hipMemcpyHostToDevice));
    d_out.alloc(129L * n);
    double *d_r = d_out.p, *d_J = d_r + 8L * n, *d_rho = d_J + 120L * n;
    hipLaunchKernelGGL(arslam::k_debug_rj_loss, arslam::blocks_of_128(8L * n), dim3(128), 0, 0, n, d_in.p,
                       d_in.p + 3L * n, d_in.p + 9L * n, d_in.p + 15L * n, d_k.p, d_in.p + 23L * n, d_r, d_J, d_rho);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    arslam::download(r, d_r, 8L * n);
    arslam::download(J, d_J, 120L * n);
    arslam::download(rho, d_rho, n);
  });
}

extern "C" int arslam_debug_angle_axis_rotate(int n, const double *w, const double *p, double *out,
                                              int *branch) {
  if (n < 0 || (n && (!w || !p || !out || !branch))) return ARSLAM_E_INVALID_ARG;
  if (n == 0) return ARSLAM_OK;
  return arslam::api_guarded([&] {
    DevBuf<double> d;   // w [3 n] | p [3 n] | out [3 n]
    DevBuf<int> d_b;
    d.alloc(9L * n);
    d_b.alloc(n);
    HIP_CHECK(hipMemcpy(d.p, w, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d.p + 3L * n, p, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(arslam::k_debug_aa, arslam::blocks_of_128(n), dim3(128), 0, 0, n, d.p, d.p + 3L * n,
                       d.p + 6L * n, d_b.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    arslam::download(out, d.p + 6L * n, 3L * n);
    arslam::download(branch, d_b.p, n);
  });
}
