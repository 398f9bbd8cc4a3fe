// lm_evaluate.h -- what arslam_lm_evaluate's kernels (lm_evaluate.hip) take:
// the problem's structure in the caller's order and the call's buffers, in a
// struct of its own.  Nothing here is part of DevProblem, so no solver kernel's
// arguments (and none of their code) change with it.
#pragma once

namespace arslam {

// The per-observation store of k_eval_obs, SoA over the n_obs observations
// (item i of observation o at obs[i * n_obs + o]): the 15 products J~'r~ of the
// observation's columns [f, l1, l2 | capture 6 | tag 6], then s, rho', rho.
constexpr int kEvalGrad = 15;
constexpr int kEvalS = 15, kEvalW = 16, kEvalRho = 17;
constexpr int kEvalItems = 18;
// The fixed trees over all observations (camera f, l1, l2 and the cost): one
// partial per kEvalTreeBlock consecutive observations, then one block over the
// partials.  Constants of the code: the sums' bits depend on n_obs alone.
constexpr int kEvalTreeBlock = 256;
constexpr int kEvalTreeSums = 4;
// k_eval_obs: four wavefronts of 8 observations each per block
constexpr int kEvalObsBlock = 256;

struct EvalProblem {
  int nc = 0, nt = 0, nb = 0;
  // the structure, uploaded once per loaded problem
  const int *obs_cap = nullptr, *obs_tag = nullptr;   // [nb]
  const double *corners = nullptr;                    // [8 nb]
  const unsigned char *loss_kind = nullptr;           // [nb] (a problem with losses)
  const double *loss_a = nullptr;
  const double *obs_size = nullptr;                   // [nb] (a problem with a side other than the default)
  // block b's observations, ascending: items[start[b] .. start[b + 1]); the
  // captures are blocks 0 .. nc - 1, the tags nc .. nc + nt - 1
  const int *blk_start = nullptr;                     // [nc + nt + 1]
  const int *blk_items = nullptr;                     // [2 nb]
  const unsigned char *blk_const = nullptr;           // [nc + nt]
  int camera_const = 0;
  // the call's buffers
  const double *x = nullptr;    // [3 + 6 nc + 6 nt] camera | captures | tags
  double *residuals = nullptr;  // [8 nb], or null: not stored
  double *obs = nullptr;        // [kEvalItems nb]
  double *parts = nullptr;      // [kEvalTreeSums * ceil(nb / kEvalTreeBlock)]
  double *out = nullptr;        // [1 + 3 + 6 nc + 6 nt] cost | gradient
};

}  // namespace arslam
