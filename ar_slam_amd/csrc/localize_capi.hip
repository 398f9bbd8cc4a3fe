// localize_capi.hip -- the batched localizer's handle (its device buffers, losses
// and covariance outputs) and the C-ABI of include/arslam_localize.h over it; the
// kernels it launches are localize.hip's (localize.h).
#include "hip_host.h"
#include "localize.h"
#include "loss.h"

#include <algorithm>
#include <vector>

struct arslam_localizer {
  arslam_lm_options opt;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int nq = 0, nt = 0, nb = 0, init_from_map = 0, max_k = 0;
  bool has_tim = false, loaded = false;
  arslam::DevBuf<double> cam, tag, corners, pose_in, pose_out, aw;
  arslam::DevBuf<int> qs, ot;
  arslam::DevBuf<unsigned char> tim;
  // The map tags' sides.  The default (set_tag_size) holds for every tag of a
  // batch loaded without an array; they are bound at the load.  has_size: some
  // tag of the loaded batch has a side other than ARSLAM_DEFAULT_TAG_SIZE
  // (else nothing is uploaded and the kernels run as without sizes).
  double def_tag_size = ARSLAM_DEFAULT_TAG_SIZE;
  bool has_size = false;
  arslam::DevBuf<double> tsize;
  // The camera model (set_camera_model): which instances solve(),
  // observation_terms() and covariance() launch; l1 and l2 are the loaded
  // batch's camera[1], camera[2].
  int camera_model = ARSLAM_CAMERA_PINHOLE;
  arslam::DevBuf<arslam_localize_result> res;
  // Robust losses.  The default (set_loss) holds for every observation of a
  // batch loaded without arrays; a batch's own arrays (load_loss) override it.
  // The device copy is made by the next solve (loss_dirty), so set_loss needs
  // no reload; lk / la then stay what the last solve used (observation_terms).
  int loss_kind = ARSLAM_LOSS_NONE;
  double loss_a = 0.0;
  std::vector<unsigned char> obs_kind;   // the loaded batch's arrays, empty = the default
  std::vector<double> obs_a;
  bool has_obs_loss = false, loss_dirty = true, any_loss = false, solved = false;
  arslam::DevBuf<unsigned char> lk;
  arslam::DevBuf<double> la, terms;
  arslam::DevBuf<double> cov, cov_piv;   // covariance(): allocated by its first call
  arslam::DevBuf<int> cov_st;

  ~arslam_localizer() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }

  void ensure_stream() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
      throw arslam::ApiError(ARSLAM_E_NO_DEVICE, "no HIP device");
    int cur = -1;   // (set only when it differs)
    HIP_CHECK(hipGetDevice(&cur));
    if (opt.device >= 0 && opt.device != cur) HIP_CHECK(hipSetDevice(opt.device));
    if (!stream) {
      HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      // (timing only: no system-scope fence at the records)
      HIP_CHECK(hipEventCreateWithFlags(&ev0, hipEventDisableSystemFence));
      HIP_CHECK(hipEventCreateWithFlags(&ev1, hipEventDisableSystemFence));
    }
  }

  // (before any device call: a host without a GPU answers INVALID_ARG, and a
  // rejected loss leaves the handle as it was)
  static void check_loss(int kind, double a) {
    arslam::api_check(arslam::loss_valid(kind, a), ARSLAM_E_INVALID_ARG,
                      "loss: unknown kind, or a scale that is not finite and > 0");
  }

  // kinds / scales [n_obs]: the batch's own losses, both null = the handle's default;
  // tag_size [n_tag]: the map tags' sides, null = the handle's default for every tag
  void load(const arslam_localize_batch *b, const unsigned char *kinds = nullptr, const double *scales = nullptr,
            const double *tag_size = nullptr) {
    using arslam::api_check;
    api_check(b != nullptr, ARSLAM_E_INVALID_ARG, "null batch");
    api_check(b->n_query >= 0 && b->n_tag >= 0 && b->n_obs >= 0, ARSLAM_E_INVALID_ARG, "negative sizes");
    if (tag_size)
      for (int t = 0; t < b->n_tag; ++t)
        api_check(ARSLAM_TAG_SIZE_VALID(tag_size[t]), ARSLAM_E_INVALID_ARG, "tag_size: finite and > 0 (metres)");
    api_check((kinds == nullptr) == (scales == nullptr), ARSLAM_E_INVALID_ARG,
              "obs_loss_kind and obs_loss_a: both or neither");
    if (kinds)
      for (int o = 0; o < b->n_obs; ++o) check_loss(kinds[o], scales[o]);
    api_check(b->camera && b->pose && (!b->n_tag || b->tag) && b->query_start, ARSLAM_E_INVALID_ARG,
              "null arrays");
    api_check(!b->n_obs || (b->obs_tag && b->corners), ARSLAM_E_INVALID_ARG, "null observation arrays");
    api_check(b->query_start[0] == 0 && b->query_start[b->n_query] == b->n_obs, ARSLAM_E_INVALID_ARG,
              "query_start must run from 0 to n_obs");
    for (int q = 0; q < b->n_query; ++q) {
      api_check(b->query_start[q + 1] >= b->query_start[q], ARSLAM_E_INVALID_ARG, "query_start not monotone");
      api_check(b->query_start[q + 1] - b->query_start[q] <= ARSLAM_LOC_MAX_OBS, ARSLAM_E_UNSUPPORTED,
                "more than 64 observations in one query");
    }
    for (int o = 0; o < b->n_obs; ++o)
      api_check(b->obs_tag[o] >= 0 && b->obs_tag[o] < b->n_tag, ARSLAM_E_INVALID_ARG, "obs_tag out of range");
    ensure_stream();
    loaded = solved = false;
    has_obs_loss = kinds != nullptr;
    obs_kind.assign(kinds, kinds + (kinds ? b->n_obs : 0));
    obs_a.assign(scales, scales + (kinds ? b->n_obs : 0));
    loss_dirty = true;
    nq = b->n_query; nt = b->n_tag; nb = b->n_obs; init_from_map = b->init_from_map != 0;
    max_k = 0;
    for (int q = 0; q < nq; ++q) max_k = std::max(max_k, b->query_start[q + 1] - b->query_start[q]);
    auto up = [&](auto &buf, const auto *src, size_t count) {
      buf.alloc(std::max<size_t>(count, 1));
      buf.upload(src, count, stream);
    };
    up(cam, b->camera, 3);
    up(tag, b->tag, 6L * nt);
    up(qs, b->query_start, (size_t)nq + 1);
    up(ot, b->obs_tag, nb);
    up(corners, b->corners, 8L * nb);
    up(pose_in, b->pose, 6L * nq);
    has_tim = b->tag_in_map != nullptr;
    if (has_tim) up(tim, b->tag_in_map, nt);
    const std::vector<double> sizes = tag_size ? std::vector<double>(tag_size, tag_size + nt)
                                               : std::vector<double>((size_t)nt, def_tag_size);
    has_size = std::any_of(sizes.begin(), sizes.end(), [](double v) { return v != ARSLAM_DEFAULT_TAG_SIZE; });
    if (has_size) up(tsize, sizes.data(), (size_t)nt);   // (the sync below: sizes is a local)
    pose_out.alloc(std::max(6L * nq, 1L));
    aw.alloc(std::max(16L * nt, 1L));
    res.alloc(std::max(nq, 1));
    HIP_CHECK(hipStreamSynchronize(stream));
    loaded = true;
  }

  // The device's per-observation losses for the next solve: the batch's own or
  // the default for all; none uploaded (any_loss = false) when every kind is NONE.
  void refresh_loss() {
    if (!loss_dirty) return;
    const std::vector<unsigned char> k =
        has_obs_loss ? obs_kind : std::vector<unsigned char>((size_t)nb, (unsigned char)loss_kind);
    any_loss = std::any_of(k.begin(), k.end(), [](unsigned char v) { return v != ARSLAM_LOSS_NONE; });
    if (any_loss) {
      const std::vector<double> a = has_obs_loss ? obs_a : std::vector<double>((size_t)nb, loss_a);
      lk.alloc(nb);
      la.alloc(nb);
      lk.upload(k.data(), nb, stream);
      la.upload(a.data(), nb, stream);
      HIP_CHECK(hipStreamSynchronize(stream));   // (k, a are locals)
    }
    loss_dirty = false;
  }

  void set_loss(int kind, double a) {
    check_loss(kind, a);
    loss_kind = kind;
    loss_a = a;
    loss_dirty = true;
  }

  // s = |r|^2 and w = rho'(s) of every observation at the last solve's poses
  void observation_terms(double *sq_host, double *w_host) {
    arslam::api_check(loaded && solved, ARSLAM_E_STATE, "observation_terms needs a completed solve");
    if (!nb || (!sq_host && !w_host)) return;
    terms.alloc(2L * nb);
    arslam::launch_localize_terms(params(), terms.p, terms.p + nb, stream);
    HIP_CHECK(hipGetLastError());
    if (sq_host)
      HIP_CHECK(hipMemcpyAsync(sq_host, terms.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (w_host)
      HIP_CHECK(hipMemcpyAsync(w_host, terms.p + nb, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }

  // k_localize's arguments: the loaded batch, the options and the resident losses
  arslam::LocParams params() const {
    arslam::LocParams p{};
    p.lk = any_loss ? lk.p : nullptr;
    p.la = any_loss ? la.p : nullptr;
    p.nq = nq; p.cam = cam.p; p.tag = tag.p; p.tim = has_tim ? tim.p : nullptr;
    p.qs = qs.p; p.ot = ot.p; p.corners = corners.p; p.pose_in = pose_in.p; p.pose_out = pose_out.p;
    p.res = res.p; p.init_from_map = init_from_map; p.max_k = max_k;
    p.aw = aw.p; p.nt = nt;
    p.tsize = has_size ? tsize.p : nullptr;
    p.dist = camera_model == ARSLAM_CAMERA_RADIAL ? 1 : 0;
    p.max_iters = opt.max_num_iterations; p.max_invalid = opt.max_num_consecutive_invalid_steps;
    p.jacobi = opt.jacobi_scaling;
    p.ftol = opt.function_tolerance; p.gtol = opt.gradient_tolerance; p.ptol = opt.parameter_tolerance;
    p.r0 = opt.initial_trust_region_radius; p.rmax = opt.max_trust_region_radius;
    p.rmin = opt.min_trust_region_radius; p.min_rel = opt.min_relative_decrease;
    p.dmin = opt.min_lm_diagonal; p.dmax = opt.max_lm_diagonal;
    return p;
  }

  // cov (J~'J~)^-1 [nq*36], its status and min_pivot [nq] at the last solve's
  // poses, under the losses that solve used (lk / la as they are resident);
  // *kernel_ms (nullable): the device time of the covariance kernel
  void covariance(double *cov_host, int *status_host, double *pivot_host, double *kernel_ms = nullptr) {
    arslam::api_check(loaded && solved, ARSLAM_E_STATE, "covariance needs a completed solve");
    if (kernel_ms) *kernel_ms = 0.0;
    if (!nq || (!cov_host && !status_host && !pivot_host)) return;
    if (cov.n < 36 * (size_t)nq) {   // sized on first use, and again for a larger batch (the buffers only grow)
      cov.alloc(36 * (size_t)nq);
      cov_piv.alloc(nq);
      cov_st.alloc(nq);
    }
    arslam::LocCovParams cp{params(), cov.p, cov_st.p, cov_piv.p};
    HIP_CHECK(hipEventRecord(ev0, stream));
    arslam::launch_localize_cov(cp, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev1, stream));
    if (cov_host)
      HIP_CHECK(hipMemcpyAsync(cov_host, cov.p, 36 * (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (status_host)
      HIP_CHECK(hipMemcpyAsync(status_host, cov_st.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, stream));
    if (pivot_host)
      HIP_CHECK(hipMemcpyAsync(pivot_host, cov_piv.p, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (kernel_ms) {
      float ms = 0.0f;
      HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
      *kernel_ms = ms;
    }
  }

  void solve(double *pose_host, arslam_localize_result *res_host, double *kernel_ms) {
    arslam::api_check(loaded, ARSLAM_E_STATE, "no batch loaded");
    refresh_loss();
    const arslam::LocParams p = params();
    HIP_CHECK(hipEventRecord(ev0, stream));
    arslam::launch_localize(p, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev1, stream));
    if (pose_host && nq)
      HIP_CHECK(hipMemcpyAsync(pose_host, pose_out.p, 6L * nq * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (res_host && nq)
      HIP_CHECK(hipMemcpyAsync(res_host, res.p, (size_t)nq * sizeof(arslam_localize_result),
                               hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    solved = true;
    if (kernel_ms) {
      float ms = 0.0f;
      HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
      *kernel_ms = ms;
    }
  }
};

extern "C" {

int arslam_localizer_create(arslam_localizer **out, const arslam_lm_options *opt) {
  if (!out) return ARSLAM_E_INVALID_ARG;
  *out = nullptr;
  return arslam::api_guarded([&] {
    auto *h = new arslam_localizer();
    if (opt) h->opt = *opt; else arslam_lm_options_init(&h->opt);
    *out = h;
  });
}

void arslam_localizer_destroy(arslam_localizer *h) { delete h; }

int arslam_localizer_load(arslam_localizer *h, const arslam_localize_batch *b) {
  if (!h || !b) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->load(b); });
}

int arslam_localizer_solve(arslam_localizer *h, double *pose_out, arslam_localize_result *res,
                           double *kernel_ms) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->solve(pose_out, res, kernel_ms); });
}

int arslam_localizer_set_loss(arslam_localizer *h, int kind, double a) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->set_loss(kind, a); });
}

int arslam_localizer_get_loss(const arslam_localizer *h, int *kind, double *a) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  if (kind) *kind = h->loss_kind;
  if (a) *a = h->loss_a;
  return ARSLAM_OK;
}

int arslam_localizer_load_loss(arslam_localizer *h, const arslam_localize_batch *b,
                               const unsigned char *obs_loss_kind, const double *obs_loss_a) {
  if (!h || !b) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->load(b, obs_loss_kind, obs_loss_a); });
}

int arslam_localizer_set_tag_size(arslam_localizer *h, double size) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    arslam::api_check(ARSLAM_TAG_SIZE_VALID(size), ARSLAM_E_INVALID_ARG, "tag size: finite and > 0 (metres)");
    h->def_tag_size = size;
  });
}

int arslam_localizer_get_tag_size(const arslam_localizer *h, double *size) {
  if (!h || !size) return ARSLAM_E_INVALID_ARG;
  *size = h->def_tag_size;
  return ARSLAM_OK;
}

int arslam_localizer_set_camera_model(arslam_localizer *h, int model) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    arslam::api_check(ARSLAM_CAMERA_MODEL_VALID(model), ARSLAM_E_INVALID_ARG,
                      "camera model: ARSLAM_CAMERA_PINHOLE or ARSLAM_CAMERA_RADIAL");
    if (model == h->camera_model) return;
    h->camera_model = model;
    h->solved = false;   // (the resident poses and results are the other model's)
  });
}

int arslam_localizer_camera_model(const arslam_localizer *h, int *model) {
  if (!h || !model) return ARSLAM_E_INVALID_ARG;
  *model = h->camera_model;
  return ARSLAM_OK;
}

int arslam_localizer_load_sized(arslam_localizer *h, const arslam_localize_batch *b, const double *tag_size,
                                const unsigned char *obs_loss_kind, const double *obs_loss_a) {
  if (!h || !b) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->load(b, obs_loss_kind, obs_loss_a, tag_size); });
}

int arslam_localizer_observation_terms(arslam_localizer *h, double *sq_residual, double *weight) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->observation_terms(sq_residual, weight); });
}

int arslam_localizer_covariance(arslam_localizer *h, double *cov, int *cov_status, double *min_pivot) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->covariance(cov, cov_status, min_pivot); });
}

int arslam_localizer_covariance_timed(arslam_localizer *h, double *cov, int *cov_status, double *min_pivot,
                                      double *kernel_ms) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->covariance(cov, cov_status, min_pivot, kernel_ms); });
}

int arslam_localize_many_cov(const arslam_localize_batch *b, const arslam_lm_options *opt, int kind, double a,
                             arslam_localize_result *res, double *cov, int *cov_status) {
  return arslam_localize_many_sized(b, opt, nullptr, kind, a, res, cov, cov_status);
}

int arslam_localize_many_sized(const arslam_localize_batch *b, const arslam_lm_options *opt, const double *tag_size,
                               int kind, double a, arslam_localize_result *res, double *cov, int *cov_status) {
  if (!b) return ARSLAM_E_INVALID_ARG;
  arslam_localizer *h = nullptr;
  int rc = arslam_localizer_create(&h, opt);
  if (rc) return rc;
  rc = arslam_localizer_set_loss(h, kind, a);
  if (!rc) rc = arslam_localizer_load_sized(h, b, tag_size, nullptr, nullptr);
  if (!rc) rc = arslam_localizer_solve(h, b->pose, res, nullptr);
  if (!rc && (cov || cov_status)) rc = arslam_localizer_covariance(h, cov, cov_status, nullptr);
  arslam_localizer_destroy(h);
  return rc;
}

int arslam_localize_many_loss(const arslam_localize_batch *b, const arslam_lm_options *opt, int kind, double a,
                              arslam_localize_result *res) {
  return arslam_localize_many_cov(b, opt, kind, a, res, nullptr, nullptr);
}

int arslam_localize_many(const arslam_localize_batch *b, const arslam_lm_options *opt,
                         arslam_localize_result *res) {
  return arslam_localize_many_loss(b, opt, ARSLAM_LOSS_NONE, 0.0, res);
}

}  // extern "C"