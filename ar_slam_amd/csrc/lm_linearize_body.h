// lm_linearize_body.h -- the body of k_linearize and k_linearize_est
// (lm_linearize.hip), included between each kernel's braces: the same text in
// both, so that the instances every other problem launches keep the machine
// code they had (a shared __device__ function inlined into them does not: the
// register allocation comes out differently).  In scope: the kernel's
// arguments P, x, g, colnorm, obs_tg, parts; kChunked, kLoss, kSized; and
//   kMode    0 the pinhole, 1 the radial model with l1, l2 held, 2 with them
//            estimated: fill_rows also stores the rows' l columns to jrows_l,
//            and the capture's l gradient and squared column norms go to
//            lparts[i nc + c], i = J_l1'r, J_l2'r, |J_l1|^2, |J_l2|^2
//   lparts, jrows_l   (kMode == 2; null constants otherwise)
// A capture of no observations is never in the chunked launch, and the main
// launch's chunk(0) stores its zeros.
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
    if (kMode == 2) {
      // the l columns too (jrows_l), and the capture's l sums: a wave sum over
      // the chunk's rows, the chunks added in row order (lanes 0..3 keep one each
      // in lparts, theirs alone)
      double lsum[4];
      fill_rows<kLoss, kSized, 2>(P, x, nullptr, c, o0, 8 * q0, nr, nrows, rows, P.jrows, kLoss ? ocost : nullptr, lsum,
                                  jrows_l);
#pragma unroll
      for (int i = 0; i < 4; ++i) lsum[i] = wave_sum(lsum[i]);
      if (lane < 4) {
        const double v = lane == 0 ? lsum[0] : lane == 1 ? lsum[1] : lane == 2 ? lsum[2] : lsum[3];
        double *dst = lparts + (long)lane * P.nc + c;
        *dst = q0 ? *dst + v : v;
      }
    } else {
      fill_rows<kLoss, kSized, kMode>(P, x, nullptr, c, o0, 8 * q0, nr, nrows, rows, P.jrows, kLoss ? ocost : nullptr);
    }
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
