// lm_cov_capi.hip -- the covariance entry points of include/arslam_lm.h over
// the LM handle (lm_handle.h): the array, block, pairs and block-pair calls in
// their plain, _lens and _anchored forms.  Each family's body is written once,
// for a CovForm; an entry point is its form and one call.  Launches no kernel.
#include "lm_handle.h"
#include "lm_cov_host.h"

namespace {
using CovForm = arslam_lm::CovForm;
using CovAnchor = arslam_lm::CovAnchor;

// the anchor of a pointer-keyed anchored form (arslam_lm::pk_block looks it up): null is none, the camera is refused
CovAnchor pk_anchor(const arslam_lm *h, const double *anchor) {
  CovAnchor an;
  if (!anchor) return an;
  h->pk_block(anchor, &an.kind, &an.index);
  fail_if(an.kind == ARSLAM_BLOCK_CAMERA, ARSLAM_E_INVALID_ARG, "the anchor must be a pose block, not the camera");
  return an;
}
// a pointer-keyed form's state, after its blocks (and anchor) were looked up
void pk_check_solved(const arslam_lm *h, const std::string &who) {
  fail_if(!h->pk_loaded || h->pk_dirty, ARSLAM_E_STATE, who + ": no completed arslam_lm_solve of the problem as it stands");
}

// The array forms: compute, keep, copy out (var_f: the plain form's camera output; cov_cam, cam_status: the others').
int cov_arrays(arslam_lm *h, const CovForm &form, double *cov_cap, double *cov_tag, double *var_f, double *cov_cam,
               int *cap_status, int *tag_status, int *cam_status, arslam_lm_cov_info *info) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    h->covariance(form);
    if (cov_cap && !h->cov_cap.empty()) std::memcpy(cov_cap, h->cov_cap.data(), h->cov_cap.size() * sizeof(double));
    if (cov_tag && !h->cov_tag.empty()) std::memcpy(cov_tag, h->cov_tag.data(), h->cov_tag.size() * sizeof(double));
    if (var_f) *var_f = h->cov_var_f;
    if (cov_cam) std::memcpy(cov_cam, h->cov_cam, 9 * sizeof(double));
    if (cap_status && !h->cov_cap_status.empty())
      std::memcpy(cap_status, h->cov_cap_status.data(), h->cov_cap_status.size() * sizeof(int));
    if (tag_status && !h->cov_tag_status.empty())
      std::memcpy(tag_status, h->cov_tag_status.data(), h->cov_tag_status.size() * sizeof(int));
    if (cam_status) *cam_status = h->cov_cam_status;
    if (info) *info = h->cov_info;
  });
}

// The block forms: one block of the kept result of this form (an anchored
// form: of this anchor), computed first when another is kept or none.
int cov_block(arslam_lm *h, CovForm form, const double *anchor, const double *block, double *cov, int *status) {
  if (!h || !block || !cov) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    int kind = 0, i = 0;
    h->pk_block(block, &kind, &i);
    if (form.anchored) form.anchor = pk_anchor(h, anchor);
    const std::string who = form.name("covariance_block");
    pk_check_solved(h, who);
    if (!h->cov_kept || !(h->cov_form == form)) h->covariance(form);
    if (kind == ARSLAM_BLOCK_CAMERA && form.lens) {
      std::memcpy(cov, h->cov_cam, 9 * sizeof(double));
      if (status) *status = h->cov_cam_status;
      return;
    }
    if (kind == ARSLAM_BLOCK_CAMERA) {   // the plain form: var(f) at [0]; its status from var(f), not cov_cam_status
      std::fill(cov, cov + 9, 0.0);
      cov[0] = h->cov_var_f;
      const bool ok = h->cov_var_f >= 0.0;
      if (!ok) std::fill(cov, cov + 9, -1.0);
      const bool deficient = h->cov_info.status == ARSLAM_COV_RANK_DEFICIENT && !h->constant.count(h->camera_ptr);
      if (status) *status = ok ? ARSLAM_COV_OK : deficient ? ARSLAM_COV_RANK_DEFICIENT : ARSLAM_COV_UNAVAILABLE;
      return;
    }
    const bool is_cap = kind == ARSLAM_BLOCK_CAPTURE;
    const std::vector<double> &c = is_cap ? h->cov_cap : h->cov_tag;
    const std::vector<int> &st = is_cap ? h->cov_cap_status : h->cov_tag_status;
    fail_if((size_t)i >= st.size(), ARSLAM_E_STATE, who + ": the block is not part of the solved problem");
    std::memcpy(cov, c.data() + 36L * i, 36 * sizeof(double));
    if (status) *status = st[i];
  });
}

// The block-pair forms: one pair through covariance_pairs, in Ceres' shapes:
// rows of a by columns of b, the camera block 3 wide.  The plain form's focal
// is one row / column of the pair (l1 / l2 rows and columns 0); the others'
// camera is the top-left of the 6x6.
int cov_block_pair(arslam_lm *h, CovForm form, const double *anchor, const double *block_a, const double *block_b,
                   double *cov, int *status) {
  if (!h || !block_a || !block_b || !cov) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    arslam_lm_cov_pair pr{};
    h->pk_block(block_a, &pr.kind_a, &pr.index_a);
    h->pk_block(block_b, &pr.kind_b, &pr.index_b);
    if (form.anchored) form.anchor = pk_anchor(h, anchor);
    pk_check_solved(h, form.name("covariance_block_pair"));
    double c[36];
    int st = ARSLAM_COV_UNAVAILABLE;
    h->covariance_pairs(form, &pr, 1, c, &st, nullptr);
    const int ra = pr.kind_a == ARSLAM_BLOCK_CAMERA ? 3 : 6, cb = pr.kind_b == ARSLAM_BLOCK_CAMERA ? 3 : 6;
    if (st != ARSLAM_COV_OK) {
      std::fill(cov, cov + ra * cb, -1.0);
    } else if (form.lens || (ra == 6 && cb == 6)) {
      for (int r = 0; r < ra; ++r) std::copy(c + 6 * r, c + 6 * r + cb, cov + cb * r);
    } else {
      std::fill(cov, cov + ra * cb, 0.0);
      if (ra == 3 && cb == 6) std::copy(c, c + 6, cov);                         // row 0: cov(f, b)
      else if (ra == 6) for (int r = 0; r < 6; ++r) cov[3 * r] = c[r];          // column 0: cov(a, f)
      else cov[0] = c[0];
    }
    if (status) *status = st;
  });
}

int cov_pairs(arslam_lm *h, const CovForm &form, const arslam_lm_cov_pair *pairs, int n_pairs, double *cov, int *status,
              arslam_lm_cov_info *info) {
  if (!h || n_pairs < 0 || (n_pairs > 0 && (!pairs || !cov))) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->covariance_pairs(form, pairs, n_pairs, cov, status, info); });
}
}  // namespace

extern "C" {

int arslam_lm_covariance(arslam_lm *h, double *cov_cap, double *cov_tag, double *var_f, int *cap_status,
                         int *tag_status, arslam_lm_cov_info *info) {
  return cov_arrays(h, CovForm{}, cov_cap, cov_tag, var_f, nullptr, cap_status, tag_status, nullptr, info);
}

int arslam_lm_covariance_lens(arslam_lm *h, double *cov_cap, double *cov_tag, double *cov_cam, int *cap_status,
                              int *tag_status, int *cam_status, arslam_lm_cov_info *info) {
  return cov_arrays(h, CovForm::with_lens(), cov_cap, cov_tag, nullptr, cov_cam, cap_status, tag_status, cam_status, info);
}

int arslam_lm_covariance_anchored(arslam_lm *h, int anchor_kind, int anchor_index, double *cov_cap, double *cov_tag,
                                  double *cov_cam, int *cap_status, int *tag_status, int *cam_status,
                                  arslam_lm_cov_info *info) {
  return cov_arrays(h, CovForm::anchored_at(CovAnchor{anchor_kind, anchor_index}), cov_cap, cov_tag, nullptr, cov_cam,
                    cap_status, tag_status, cam_status, info);
}

int arslam_lm_covariance_block(arslam_lm *h, const double *block, double *cov, int *status) {
  return cov_block(h, CovForm{}, nullptr, block, cov, status);
}

int arslam_lm_covariance_block_lens(arslam_lm *h, const double *block, double *cov, int *status) {
  return cov_block(h, CovForm::with_lens(), nullptr, block, cov, status);
}

int arslam_lm_covariance_block_anchored(arslam_lm *h, const double *anchor, const double *block, double *cov,
                                        int *status) {
  return cov_block(h, CovForm::anchored_at(CovAnchor{}), anchor, block, cov, status);
}

int arslam_lm_covariance_pairs(arslam_lm *h, const arslam_lm_cov_pair *pairs, int n_pairs, double *cov, int *status,
                               arslam_lm_cov_info *info) {
  return cov_pairs(h, CovForm{}, pairs, n_pairs, cov, status, info);
}

int arslam_lm_covariance_pairs_lens(arslam_lm *h, const arslam_lm_cov_pair *pairs, int n_pairs, double *cov,
                                    int *status, arslam_lm_cov_info *info) {
  return cov_pairs(h, CovForm::with_lens(), pairs, n_pairs, cov, status, info);
}

int arslam_lm_covariance_pairs_anchored(arslam_lm *h, int anchor_kind, int anchor_index,
                                        const arslam_lm_cov_pair *pairs, int n_pairs, double *cov, int *status,
                                        arslam_lm_cov_info *info) {
  return cov_pairs(h, CovForm::anchored_at(CovAnchor{anchor_kind, anchor_index}), pairs, n_pairs, cov, status, info);
}

int arslam_lm_covariance_block_pair(arslam_lm *h, const double *block_a, const double *block_b, double *cov,
                                    int *status) {
  return cov_block_pair(h, CovForm{}, nullptr, block_a, block_b, cov, status);
}

int arslam_lm_covariance_block_pair_lens(arslam_lm *h, const double *block_a, const double *block_b, double *cov,
                                         int *status) {
  return cov_block_pair(h, CovForm::with_lens(), nullptr, block_a, block_b, cov, status);
}

int arslam_lm_covariance_block_pair_anchored(arslam_lm *h, const double *anchor, const double *block_a,
                                             const double *block_b, double *cov, int *status) {
  return cov_block_pair(h, CovForm::anchored_at(CovAnchor{}), anchor, block_a, block_b, cov, status);
}

int arslam_lm_debug_cov_camera_rows(arslam_lm *h, long n_cols, double *rows, int *row_slot) {
  if (!h || !rows) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    const CovForm form = CovForm::with_lens();
    h->cov_check_state("cov_camera_rows", form);
    fail_if(!h->has_f || h->P.cam_row < 0, ARSLAM_E_STATE, "cov_camera_rows: a problem loaded with a free camera");
    fail_if(n_cols != h->nR + 1, ARSLAM_E_INVALID_ARG, "cov_camera_rows: n_cols must be the reduced row count + 1");
    h->cov_kept = false;
    // the covariance's linearization, elimination, border and gathers, the rows read before the factorization
    arslam_lm::CovFactor cf;
    h->cov_factor(cf, form, h->block_map(), true);
    fail_if(!cf.factored, ARSLAM_E_STATE, "cov_camera_rows: the problem has no gauge anchor");
    DevBuf<double> d_out;
    d_out.alloc(3 * n_cols);
    arslam::debug_cam_rows(h->P, h->Sp, d_out.p, h->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(rows, d_out.p, 3 * n_cols * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (row_slot)
      for (int b = 0; b < 3; ++b) row_slot[b] = h->lay.row_slot[h->P.cam_row + b];
  });
}

}  // extern "C"

namespace arslam {
bool kept_anchored_cov_info(const arslam_lm *h, arslam_lm_cov_info *info) {
  if (!h || !h->cov_kept || !h->cov_form.anchored) return false;
  if (info) *info = h->cov_info;
  return true;
}
}  // namespace arslam
