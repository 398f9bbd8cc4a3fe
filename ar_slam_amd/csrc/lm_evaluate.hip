// lm_evaluate.hip -- arslam_lm_evaluate, _evaluate_blocks, _gradient_block:
// ceres::Problem::Evaluate (Ceres 2.0, default EvaluateOptions) for the mapper.
//
// A path of its own beside the solver's.  The problem's structure lives on the
// device in the caller's order (EvalProblem, lm_evaluate.h), uploaded at the
// first evaluate after a load or an added block; a call uploads the parameter
// vector [camera 3 | captures 6 n_cap | tags 6 n_tag] and runs
//
//   k_eval_obs      lane = residual row, 8 observations per wavefront: the row
//                   evaluators of the solver (residual_jacobian_row,
//                   robustify_row, the l columns as fill_rows forms them), the
//                   rows summed per observation by obs_sum8 -- s, and the 15
//                   products J~'r~ of the observation's columns.  Stores the
//                   corrected residuals coalesced, and per observation the 15
//                   contributions, s, rho' and rho (SoA, kEvalItems arrays).
//   k_eval_blocks   one thread per entry of a capture's or a tag's gradient:
//                   the sum of its observations' contributions in ascending
//                   observation order; exactly 0.0 for a constant block (and for
//                   a block without observations: an empty sum).
//   k_eval_tree     the camera's three entries and the cost: a fixed pairwise
//                   tree over every kEvalTreeBlock consecutive observations,
//                   then the same tree over the partials in one block.
//
// No atomics; every sum's order is a function of the problem alone, so two
// calls, and handles that differ in any solver option, give the same bits.
// Nothing here reads or writes DevProblem or any of the solver's buffers.
#include "lm_handle.h"
#include "lm_rows.h"

namespace arslam {

namespace {

// kLoss: the problem has a loss other than NONE (EvalProblem::loss_*), and the
// call applies it; kSized: a tag side other than the default (obs_size);
// kMode: 0 the pinhole, 1 the radial model with l1, l2 held, 2 with them
// estimated (the row's two l columns, corrected like the rest of the row).
template <bool kLoss, bool kSized, int kMode>
__global__ __launch_bounds__(kEvalObsBlock) void k_eval_obs(const EvalProblem E) {
  const long gid = (long)blockIdx.x * kEvalObsBlock + threadIdx.x;
  const long o = gid >> 3;
  // (the rows past 8 n_obs neither load nor store; an observation's 8 lanes
  // leave or stay together, so obs_sum8's partners are always active)
  if (o >= E.nb) return;
  const int row = (int)(gid & 7), corner = row >> 1, comp = row & 1;
  const int c = E.obs_cap[o], t = E.obs_tag[o];
  const double *cam = E.x;
  const double *cap = E.x + 3 + 6L * c;
  const double *tag = E.x + 3 + 6L * E.nc + 6L * t;
  const double half = kSized ? 0.5 * E.obs_size[o] : kArucoHalf;
  double J[13], Jl[2] = {0.0, 0.0};
  double r = residual_jacobian_row<kMode != 0>(cam, cap, tag, half, corner, comp, E.corners[gid], J,
                                               kMode == 2 ? Jl : nullptr);
  const double s = obs_sum8(r * r);
  double rho = s, rho1 = 1.0;
  if (kLoss) {
    const int kind = E.loss_kind[o];
    const double a = E.loss_a[o];
    loss_eval(kind, a, s, &rho, &rho1);
    double w = 1.0;
    robustify_row(kind, a, r, J, &w);
    if (kMode == 2) { Jl[0] *= w; Jl[1] *= w; }
  }
  if (E.residuals) E.residuals[gid] = r;
  // the observation's items: every one of its 8 lanes holds the same bits of
  // each sum, and lane `row` stores items row, row + 8 and row + 16
  double it0 = 0.0, it1 = 0.0, it2 = 0.0;
#pragma unroll
  for (int j = 0; j < kEvalGrad; ++j) {
    double p = 0.0;
    if (j == 0) p = obs_sum8(J[0] * r);
    else if (j < 3) p = kMode == 2 ? obs_sum8(Jl[j - 1] * r) : 0.0;
    else p = obs_sum8(J[j - 2] * r);
    if ((j & 7) == row) {
      if (j < 8) it0 = p; else it1 = p;
    }
  }
  if (row == 7) it1 = s;      // kEvalS = 15
  if (row == 0) it2 = rho1;   // kEvalW = 16
  if (row == 1) it2 = rho;    // kEvalRho = 17
  double *dst = E.obs + o;
  dst[(long)row * E.nb] = it0;
  dst[(long)(row + 8) * E.nb] = it1;
  if (row + 16 < kEvalItems) dst[(long)(row + 16) * E.nb] = it2;
}

// entry j of block b (captures, then tags): out[1 + 3 + 6 b + j]
__global__ __launch_bounds__(256) void k_eval_blocks(const EvalProblem E) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long b = gid / 6;
  if (b >= (long)E.nc + E.nt) return;
  const int j = (int)(gid - 6 * b);
  const double *src = E.obs + (long)((b < E.nc ? 3 : 9) + j) * E.nb;
  double acc = 0.0;
  const int i1 = E.blk_start[b + 1];
  // (unrolled: four entries' loads in flight, the adds still in list order)
#pragma unroll 4
  for (int i = E.blk_start[b]; i < i1; ++i) acc += src[E.blk_items[i]];
  E.out[4 + 6 * b + j] = E.blk_const[b] ? 0.0 : acc;
}

// The four sums over all observations (f, l1, l2 contributions and rho).
// kFinal = false: block i's pairwise tree over observations
// [i kEvalTreeBlock, (i + 1) kEvalTreeBlock), zeros past n_obs, to parts.
// true (one block): thread t adds parts t, t + kEvalTreeBlock, ... in that
// order, then the same tree; thread 0 stores the cost and the camera's entries.
template <bool kFinal>
__global__ __launch_bounds__(kEvalTreeBlock) void k_eval_tree(const EvalProblem E, int nparts) {
  __shared__ double red[kEvalTreeSums][kEvalTreeBlock];
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < kEvalTreeSums; ++q) {
    double v = 0.0;
    if (!kFinal) {
      const long o = (long)blockIdx.x * kEvalTreeBlock + t;
      if (o < E.nb) v = E.obs[(long)(q < 3 ? q : kEvalRho) * E.nb + o];
    } else {
      for (int i = t; i < nparts; i += kEvalTreeBlock) v += E.parts[(long)q * nparts + i];
    }
    red[q][t] = v;
  }
  __syncthreads();
  for (int off = kEvalTreeBlock / 2; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int q = 0; q < kEvalTreeSums; ++q) red[q][t] += red[q][t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (!kFinal) {
#pragma unroll
      for (int q = 0; q < kEvalTreeSums; ++q) E.parts[(long)q * nparts + blockIdx.x] = red[q][0];
    } else {
      E.out[0] = 0.5 * red[3][0];
#pragma unroll
      for (int q = 0; q < 3; ++q) E.out[1 + q] = E.camera_const ? 0.0 : red[q][0];
    }
  }
}

template <bool kLoss, bool kSized>
void launch_eval_obs_mode(const EvalProblem &E, int mode, dim3 grid, hipStream_t s) {
  if (mode == 2) k_eval_obs<kLoss, kSized, 2><<<grid, kEvalObsBlock, 0, s>>>(E);
  else if (mode == 1) k_eval_obs<kLoss, kSized, 1><<<grid, kEvalObsBlock, 0, s>>>(E);
  else k_eval_obs<kLoss, kSized, 0><<<grid, kEvalObsBlock, 0, s>>>(E);
}

void launch_eval_obs(const EvalProblem &E, bool loss, bool sized, int mode, hipStream_t s) {
  const dim3 grid((unsigned)((8L * E.nb + kEvalObsBlock - 1) / kEvalObsBlock));
  if (loss) {
    if (sized) launch_eval_obs_mode<true, true>(E, mode, grid, s);
    else launch_eval_obs_mode<true, false>(E, mode, grid, s);
  } else {
    if (sized) launch_eval_obs_mode<false, true>(E, mode, grid, s);
    else launch_eval_obs_mode<false, false>(E, mode, grid, s);
  }
}

}  // namespace

}  // namespace arslam

// The structure of the problem as the caller numbers it: arslam_lm_load_soa*'s
// arrays (ev_src) or the pointer-keyed blocks, with each block's observation
// list, in one upload.
void arslam_lm::eval_upload_structure(bool pk) {
  const int nc_ = pk ? (int)cap_ptrs.size() : ev_src.n_cap;
  const int nt_ = pk ? (int)tag_ptrs.size() : ev_src.n_tag;
  const int nb_ = pk ? (int)pk_obs_cap.size() : ev_src.n_obs;
  const int *ocap = pk ? pk_obs_cap.data() : ev_src.obs_cap;
  const int *otag = pk ? pk_obs_tag.data() : ev_src.obs_tag;
  const double *corners = pk ? pk_corners.data() : ev_src.corners;
  fail_if(nc_ < 0 || nt_ < 0 || nb_ < 0, ARSLAM_E_INVALID_ARG, "evaluate: negative sizes");
  fail_if(nb_ > 0 && (!ocap || !otag || !corners), ARSLAM_E_INVALID_ARG, "evaluate: null observation arrays");
  for (int b = 0; b < nb_; ++b)
    fail_if(ocap[b] < 0 || ocap[b] >= nc_ || otag[b] < 0 || otag[b] >= nt_, ARSLAM_E_INVALID_ARG,
            "evaluate: the observation arrays are not the loaded problem's (index out of range)");
  // losses and sides, per observation; a problem of NONE and default sides runs the plain instances
  const unsigned char *kind = pk ? pk_loss_kind.data()
                                 : ev_src_loss_from == 1 ? ev_src_kind.data()
                                 : ev_src_loss_from == 2 ? soa_loss_kind.data() : nullptr;
  const double *la = pk ? pk_loss_a.data()
                        : ev_src_loss_from == 1 ? ev_src_a.data() : ev_src_loss_from == 2 ? soa_loss_a.data() : nullptr;
  const double *size = pk ? pk_size.data() : ev_src_sized ? soa_size.data() : nullptr;
  bool with_loss = false, with_size = false;
  for (int b = 0; b < nb_ && kind; ++b) with_loss = with_loss || kind[b] != ARSLAM_LOSS_NONE;
  for (int b = 0; b < nb_ && size; ++b) with_size = with_size || size[b] != ARSLAM_DEFAULT_TAG_SIZE;
  // each block's observations, ascending (a counting sort keeps the order)
  std::vector<int> start((size_t)nc_ + nt_ + 1, 0), items(2 * (size_t)nb_);
  for (int b = 0; b < nb_; ++b) {
    ++start[ocap[b] + 1];
    ++start[(size_t)nc_ + otag[b] + 1];
  }
  for (size_t i = 0; i + 1 < start.size(); ++i) start[i + 1] += start[i];
  {
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int b = 0; b < nb_; ++b) {
      items[fill[ocap[b]]++] = b;
      items[fill[(size_t)nc_ + otag[b]]++] = b;
    }
  }
  std::vector<unsigned char> is_const((size_t)nc_ + nt_, 0);
  bool cam_const;
  if (pk) {
    for (int c = 0; c < nc_; ++c) is_const[c] = constant.count(cap_ptrs[c]) ? 1 : 0;
    for (int t = 0; t < nt_; ++t) is_const[(size_t)nc_ + t] = constant.count(tag_ptrs[t]) ? 1 : 0;
    cam_const = constant.count(camera_ptr) != 0;
  } else {
    for (int c = 0; c < nc_ && ev_src.cap_const; ++c) is_const[c] = ev_src.cap_const[c] ? 1 : 0;
    for (int t = 0; t < nt_ && ev_src.tag_const; ++t) is_const[(size_t)nc_ + t] = ev_src.tag_const[t] ? 1 : 0;
    cam_const = ev_src.camera_const != 0;
  }
  arslam::EvalProblem E{};
  E.nc = nc_; E.nt = nt_; E.nb = nb_;
  E.camera_const = cam_const ? 1 : 0;
  ev_upload.add(const_cast<int **>(&E.obs_cap), ocap, (size_t)nb_);
  ev_upload.add(const_cast<int **>(&E.obs_tag), otag, (size_t)nb_);
  ev_upload.add(const_cast<double **>(&E.corners), corners, 8 * (size_t)nb_);
  if (with_loss) {
    ev_upload.add(const_cast<unsigned char **>(&E.loss_kind), kind, (size_t)nb_);
    ev_upload.add(const_cast<double **>(&E.loss_a), la, (size_t)nb_);
  }
  if (with_size) ev_upload.add(const_cast<double **>(&E.obs_size), size, (size_t)nb_);
  ev_upload.add(const_cast<int **>(&E.blk_start), start.data(), start.size());
  ev_upload.add(const_cast<int **>(&E.blk_items), items.data(), items.size());
  ev_upload.add(const_cast<unsigned char **>(&E.blk_const), is_const.data(), is_const.size());
  ev_upload.commit(stream);
  EV = E;
  ev_nc = nc_; ev_nt = nt_; ev_nb = nb_;
  ev_loss = with_loss;
  ev_sized = with_size;
  ev_cam_const = cam_const;
  ev_mode = camera_model == ARSLAM_CAMERA_RADIAL ? (est_active() && !cam_const ? 2 : 1) : 0;
  ev_pk = pk;
  ev_valid = true;
}

void arslam_lm::evaluate(bool pk, const arslam_lm_evaluate_options *eo, double *cost, double *residuals,
                         double *sq_norm, double *weight, double *gradient) {
  const bool apply_loss = eo ? eo->apply_loss_function != 0 : true;
  fail_if(eo && eo->apply_loss_function != 0 && eo->apply_loss_function != 1, ARSLAM_E_INVALID_ARG,
          "evaluate: apply_loss_function must be 0 or 1");
  fail_if(multi(), ARSLAM_E_UNSUPPORTED, "evaluate is single-rank only (a handle of several ranks holds a part of the problem)");
  if (pk) fail_if(pk_obs_cap.empty(), ARSLAM_E_STATE, "evaluate_blocks: no residual blocks");
  else fail_if(!loaded || pk_loaded || !ev_src_set, ARSLAM_E_STATE, "evaluate: no problem loaded by arslam_lm_load_soa");
  ensure_stream();
  if (pk) ev_grad_valid = false;
  if (!ev_valid || ev_pk != pk) eval_upload_structure(pk);
  const long n_ = 3 + 6L * ev_nc + 6L * ev_nt;
  // the parameter values as they are now
  h_ev_x.alloc(n_);
  double *hx = h_ev_x.p;
  if (pk) {
    std::memcpy(hx, camera_ptr, 3 * sizeof(double));
    for (int c = 0; c < ev_nc; ++c) std::memcpy(hx + 3 + 6L * c, cap_ptrs[c], 6 * sizeof(double));
    for (int t = 0; t < ev_nt; ++t) std::memcpy(hx + 3 + 6L * ev_nc + 6L * t, tag_ptrs[t], 6 * sizeof(double));
  } else {
    std::memcpy(hx, ev_src.camera, 3 * sizeof(double));
    if (ev_nc) std::memcpy(hx + 3, ev_src.cap, 6L * ev_nc * sizeof(double));
    if (ev_nt) std::memcpy(hx + 3 + 6L * ev_nc, ev_src.tag, 6L * ev_nt * sizeof(double));
  }
  const bool want_grad = pk || gradient != nullptr;
  const int nparts = (ev_nb + arslam::kEvalTreeBlock - 1) / arslam::kEvalTreeBlock;
  d_ev_x.alloc(n_);
  d_ev_out.alloc(1 + n_);
  d_ev_obs.alloc((size_t)arslam::kEvalItems * std::max(ev_nb, 1));
  d_ev_parts.alloc((size_t)arslam::kEvalTreeSums * std::max(nparts, 1));
  if (residuals) d_ev_res.alloc(8 * (size_t)std::max(ev_nb, 1));
  // options.phase_timing: events around the upload, each kernel and the copy back
  const bool timed = opt.phase_timing != 0;
  ev_ms_valid = false;
  const auto mark = [&](int i) {
    if (!timed) return;
    if (!ev_evt[i]) HIP_CHECK(hipEventCreate(&ev_evt[i]));
    HIP_CHECK(hipEventRecord(ev_evt[i], stream));
  };
  mark(0);
  HIP_CHECK(hipMemcpyAsync(d_ev_x.p, hx, n_ * sizeof(double), hipMemcpyHostToDevice, stream));
  mark(1);
  arslam::EvalProblem E = EV;
  E.x = d_ev_x.p;
  E.residuals = residuals ? d_ev_res.p : nullptr;
  E.obs = d_ev_obs.p;
  E.parts = d_ev_parts.p;
  E.out = d_ev_out.p;
  if (ev_nb == 0) {
    HIP_CHECK(hipMemsetAsync(d_ev_out.p, 0, (1 + n_) * sizeof(double), stream));
  } else {
    arslam::launch_eval_obs(E, ev_loss && apply_loss, ev_sized, ev_mode, stream);
    mark(2);
    if (want_grad) {
      const long entries = 6L * (ev_nc + ev_nt);
      if (entries) arslam::k_eval_blocks<<<dim3((unsigned)((entries + 255) / 256)), 256, 0, stream>>>(E);
    }
    mark(3);
    if (want_grad || cost) {
      arslam::k_eval_tree<false><<<dim3((unsigned)nparts), arslam::kEvalTreeBlock, 0, stream>>>(E, nparts);
      arslam::k_eval_tree<true><<<dim3(1), arslam::kEvalTreeBlock, 0, stream>>>(E, nparts);
    }
    mark(4);
    HIP_CHECK(hipGetLastError());
  }
  // copy back what was asked for
  double cost_v = 0.0;
  if (cost) HIP_CHECK(hipMemcpyAsync(&cost_v, d_ev_out.p, sizeof(double), hipMemcpyDeviceToHost, stream));
  if (pk) ev_grad.resize(n_);
  double *gdst = pk ? ev_grad.data() : gradient;
  if (gdst) HIP_CHECK(hipMemcpyAsync(gdst, d_ev_out.p + 1, n_ * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (ev_nb) {
    if (residuals)
      HIP_CHECK(hipMemcpyAsync(residuals, d_ev_res.p, 8L * ev_nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (sq_norm)
      HIP_CHECK(hipMemcpyAsync(sq_norm, d_ev_obs.p + (long)arslam::kEvalS * ev_nb, ev_nb * sizeof(double),
                               hipMemcpyDeviceToHost, stream));
    if (weight)
      HIP_CHECK(hipMemcpyAsync(weight, d_ev_obs.p + (long)arslam::kEvalW * ev_nb, ev_nb * sizeof(double),
                               hipMemcpyDeviceToHost, stream));
  }
  mark(5);
  HIP_CHECK(hipStreamSynchronize(stream));
  if (timed && ev_nb) {
    for (int i = 0; i < 5; ++i) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, ev_evt[i], ev_evt[i + 1]));
      ev_ms[i] = ms;
    }
    ev_ms_valid = true;
  }
  if (cost) *cost = cost_v;
  if (pk) ev_grad_valid = true;
}

extern "C" {

int arslam_lm_evaluate_options_init(arslam_lm_evaluate_options *o) {
  if (!o) return ARSLAM_E_INVALID_ARG;
  o->apply_loss_function = 1;
  return ARSLAM_OK;
}

int arslam_lm_evaluate(arslam_lm *h, const arslam_lm_evaluate_options *opt, double *cost, double *residuals,
                       double *sq_norm, double *weight, double *gradient) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->evaluate(false, opt, cost, residuals, sq_norm, weight, gradient); });
}

int arslam_lm_evaluate_blocks(arslam_lm *h, const arslam_lm_evaluate_options *opt, double *cost, double *residuals,
                              double *sq_norm, double *weight) {
  if (!h) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] { h->evaluate(true, opt, cost, residuals, sq_norm, weight, nullptr); });
}

int arslam_lm_debug_evaluate_times(arslam_lm *h, double ms[5]) {
  if (!h || !ms) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    fail_if(!h->ev_ms_valid, ARSLAM_E_STATE, "evaluate_times: no evaluate under options.phase_timing = 1 yet");
    for (int i = 0; i < 5; ++i) ms[i] = h->ev_ms[i];
  });
}

int arslam_lm_gradient_block(arslam_lm *h, const double *block, double *out) {
  if (!h || !block || !out) return ARSLAM_E_INVALID_ARG;
  return arslam::api_guarded([&] {
    int kind = 0, i = 0;
    h->pk_block(block, &kind, &i);
    fail_if(!h->ev_grad_valid, ARSLAM_E_STATE,
            "gradient_block: no arslam_lm_evaluate_blocks of the problem as it stands");
    if (kind == ARSLAM_BLOCK_CAMERA) {
      std::memcpy(out, h->ev_grad.data(), 3 * sizeof(double));
      return;
    }
    const long at = kind == ARSLAM_BLOCK_CAPTURE ? 3 + 6L * i : 3 + 6L * h->ev_nc + 6L * i;
    fail_if((size_t)at + 6 > h->ev_grad.size(), ARSLAM_E_STATE, "gradient_block: the block is not part of the evaluated problem");
    std::memcpy(out, h->ev_grad.data() + at, 6 * sizeof(double));
  });
}

}  // extern "C"
