// lm_slot_norms_body.h -- the body of k_slot_norms and k_slot_norms_l
// (lm_reduce.hip), included between each kernel's braces: the same text in
// both, so that the kernel every other problem launches keeps the machine code
// it had.  In scope: the kernel's arguments; and
//   kL     l1 and l2 are estimated: their gradient and squared column norms
//          come from lred[0..3] (k_cam_l_reduce's sums of k_linearize_est's
//          partials), as f's come from red
//   lred   (kL; a null constant otherwise)
  __shared__ double rs[6][256];
  __shared__ int last;
  const int t = threadIdx.x;
  // the camera slots from the reduced per-capture partials (f gradient and
  // column norm; l1, l2 have no Jacobian column): written once, and used here
  // in place of g[0..2]
  const double g0 = free_[0] ? red[P_GF] : 0.0;
  const double gl1 = kL && free_[1] ? lred[0] : 0.0, gl2 = kL && free_[2] ? lred[1] : 0.0;
  const double cl1 = kL && free_[1] ? lred[2] : 0.0, cl2 = kL && free_[2] ? lred[3] : 0.0;
  if (blockIdx.x == 0 && t == 0) {
    g[0] = g0;
    colnorm[0] = free_[0] ? red[P_CF] : 0.0;
    if (kL) {
      g[1] = gl1;
      g[2] = gl2;
      colnorm[1] = cl1;
      colnorm[2] = cl2;
    } else {
      g[1] = g[2] = 0.0;
      colnorm[1] = colnorm[2] = 0.0;
    }
  }
  const double cn0 = free_[0] ? red[P_CF] : 0.0;   // (colnorm[0], as block 0 writes it)
  double v[6] = {0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * 256 + t; i < n; i += (long)kNormBlocks * 256) {
    if (diag) {   // the LM diagonal of the new linearization (launch_exec_reset's k_lm_diag work)
      const double cn = i >= 3 ? colnorm[i] : (i == 0 ? cn0 : kL ? (i == 1 ? cl1 : cl2) : 0.0);
      diag[i] = fmin(fmax(scale[i] * scale[i] * cn, dmin), dmax);
    }
    // (several ranks: each slot counted on the rank holding it, DevProblem::f_own)
    if (!free_[i] || (f_own && !f_own[i])) continue;
    const int o = (i >= cap_lo && i < cap_hi) ? 0 : 3;
    const double gv = i >= 3 ? g[i] : (i == 0 ? g0 : kL ? (i == 1 ? gl1 : gl2) : 0.0), xv = x[i];
    v[o] = fmax(v[o], fabs(gv));
    v[o + 1] += gv * gv;
    v[o + 2] += xv * xv;
  }
  for (int q = 0; q < 6; ++q) rs[q][t] = v[q];
  __syncthreads();
  for (int off = 128; off >= kWave; off >>= 1) {
    if (t < off) {
      rs[0][t] = fmax(rs[0][t], rs[0][t + off]);
      rs[1][t] += rs[1][t + off];
      rs[2][t] += rs[2][t + off];
      rs[3][t] = fmax(rs[3][t], rs[3][t + off]);
      rs[4][t] += rs[4][t + off];
      rs[5][t] += rs[5][t + off];
    }
    __syncthreads();
  }
  if (t < kWave)
    for (int q = 0; q < 6; ++q) {
      const double r = (q % 3 == 0) ? wave_tree_max(rs[q][t], kWave) : wave_tree_sum(rs[q][t], kWave);
      if (t == 0) rs[q][0] = r;
    }
  // out[8 + 6 b + q]: block b's partials; out[7] (as an int): blocks done.
  // The last block to finish reduces the kNormBlocks partials over a fixed
  // tree (independent of which block is last) into out[0..5], and resets the
  // count for the next launch.
  double *part = out + 8;
  int *done = reinterpret_cast<int *>(out + 7);
  if (t == 0) {
    for (int q = 0; q < 6; ++q) part[6L * blockIdx.x + q] = rs[q][0];
    __threadfence();   // the partials before the count (agent scope: the blocks span XCDs)
    last = atomicAdd(done, 1) == kNormBlocks - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();     // every block's partials after the count
  if (t < kNormBlocks)
    for (int q = 0; q < 6; ++q) rs[q][t] = part[6L * t + q];
  __syncthreads();
  for (int off = kNormBlocks / 2; off >= kWave; off >>= 1) {
    if (t < off)
      for (int q = 0; q < 6; ++q)
        rs[q][t] = (q % 3 == 0) ? fmax(rs[q][t], rs[q][t + off]) : rs[q][t] + rs[q][t + off];
    __syncthreads();
  }
  if (t < kWave) {
    const int left = kNormBlocks < kWave ? kNormBlocks : kWave;
    double r6[6];
    for (int q = 0; q < 6; ++q) {
      const double v0 = t < left ? rs[q][t] : 0.0;
      r6[q] = (q % 3 == 0) ? wave_tree_max(v0, left) : wave_tree_sum(v0, left);
    }
    if (t == 0)
      for (int q = 0; q < 6; ++q) rs[q][0] = r6[q];
  }
  __syncthreads();
  if (t < 6) {
    out[t] = rs[t][0];
    if (hout) {
      hout[t] = rs[t][0];
      __threadfence_system();
    }
  }
  if (t == 0) atomicExch(done, 0);
  if (hout && seq > 0.0) {
    __syncthreads();
    if (t == 0) __hip_atomic_store(hout + kHostSeq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
