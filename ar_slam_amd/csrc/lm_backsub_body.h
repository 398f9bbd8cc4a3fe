// lm_backsub_body.h -- the body of k_backsub and k_backsub_est (lm_step.hip),
// included between each kernel's braces: the same text in both, so that the
// instances every other problem launches keep the machine code they had (a
// shared __device__ function inlined into them does not).  In scope: the
// kernel's arguments P, x, scale, diag, radius, yF, xc, parts, reuse_ui,
// with_cost; kChunked, kLoss, kSized, kDist; and
//   kEst      l1, l2 estimated: each row's product with the reduced solution
//             takes in the two l columns (load_rows_q<true>)
//   jrows_l   (kEst; a null constant otherwise)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  int k;
  const int c = chunk_capture<kChunked>(P, k), lane = threadIdx.x;
  if (c < 0) return;
  const int o0 = P.cap_start[c];
  const long sc = slot_cap(P, c);
  if (k == 0) {
    if (lane < 6) xc[sc + lane] = x[sc + lane];
    if (lane == 0) {
      parts[(long)P_MODEL * P.nc + c] = 0.0;
      parts[(long)P_STEP2 * P.nc + c] = 0.0;
      parts[(long)P_YBAD * P.nc + c] = 0.0;
      if (with_cost) {
        parts[(long)P_COST * P.nc + c] = 0.0;
        parts[(long)P_FIXED * P.nc + c] = 0.0;
        parts[(long)P_CBAD * P.nc + c] = 0.0;
      }
    }
    return;
  }
  const int nrows = 8 * k;
  // the rows go through LDS in chunks of one wave's 64 rows (kObsChunk
  // observations); each lane's running sum is carried over the chunks in row
  // order, as over the whole capture at once
  constexpr int kChunkRows = 8 * kObsChunk;
  double *rows = sm;
  double *qv = rows + (long)kChunkRows * kRowStride;   // [kChunkRows]
  double *U = qv + kChunkRows;                    // 36
  double *Ui = U + 36;                            // 36
  double *v = Ui + 36;                            // 8
  double *yc = v + 8;                             // 8
  const double yf = P.cam_row >= 0 ? yF[P.cam_row] : 0.0;
  const double yl1 = kEst ? yF[P.cam_row + 1] : 0.0, yl2 = kEst ? yF[P.cam_row + 2] : 0.0;   // (kEst: the camera is free)
  if (reuse_ui && lane < 36) Ui[lane] = P.cap_ui[36L * c + lane];   // (U_c + D_c^2)^{-1} as k_schur formed it
  // lanes 0..20: U = E'E (upper triangle entry (a, b)); 21..26 (32..37 with
  // the stored inverse): v = E'(b - F z); each lane's sum runs on over the
  // chunks in LDS (U, v), nothing held in registers across the row loads
  auto chunk = [&](int r0) __attribute__((always_inline)) {
    const int nr = min(kChunkRows, nrows - r0);
    if (kEst) load_rows_q<true>(P, scale, yF, yf, c, o0, r0, nr, nrows, rows, qv, yl1, yl2, jrows_l);
    else load_rows_q(P, scale, yF, yf, c, o0, r0, nr, nrows, rows, qv);
    __syncthreads();
    const int va = reuse_ui ? lane - 32 : lane - 21;
    if (!reuse_ui && lane < 21) {
      int a, b;
      upper6(lane, a, b);
      double s = r0 ? U[6 * a + b] : 0.0;
      for (int r = 0; r < nr; ++r) s += rows[(long)r * kRowStride + 1 + a] * rows[(long)r * kRowStride + 1 + b];
      U[6 * a + b] = s;
      U[6 * b + a] = s;
    } else if (va >= 0 && va < 6) {
      double s = r0 ? v[va] : 0.0;
      for (int r = 0; r < nr; ++r) {
        const double *rr = rows + (long)r * kRowStride;
        s += rr[1 + va] * (rr[13] - qv[r]);   // E'(b - F z)
      }
      v[va] = s;
    }
  };
  if (!kChunked) {   // (at most one chunk)
    chunk(0);
  } else {
    for (int r0 = 0; r0 < nrows; r0 += kChunkRows) {
      if (r0) __syncthreads();   // the previous chunk's LDS reads are done
      chunk(r0);
    }
  }
  __syncthreads();
  const bool direct = group_direct(P, c);
  if (direct) {
    // (mixed e-set) a direct group's own pose is a reduced-side block (its last
    // local block): its step is the reduced solution's, as k_update_f forms it
    if (lane < 6) {
      const int r0 = P.tag_row[P.blk_tag[P.cap_blk_start[c + 1] - 1]];
      yc[lane] = r0 >= 0 ? yF[r0 + lane] : 0.0;
    }
  } else if (reuse_ui) {
    if (lane < 6) {
      double t = 0.0;
#pragma unroll
      for (int b = 0; b < 6; ++b) t += Ui[6 * lane + b] * v[b];
      yc[lane] = t;
    }
  } else if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) U[7 * a] += lm_d2(diag, sc + a, radius);
    inv6(U, Ui);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double t = 0.0;
#pragma unroll
      for (int b = 0; b < 6; ++b) t += Ui[6 * a + b] * v[b];
      yc[a] = t;
    }
  }
  __syncthreads();
  // model cost change share: p = Jt y (= -Jt step), sum p (r - p/2) (a capture
  // of more than one chunk loads its rows again)
  double mpart = 0.0;
  auto model = [&](int nr) __attribute__((always_inline)) {
    for (int row = lane; row < nr; row += kWave) {
      const double *rr = rows + (long)row * kRowStride;
      double p = qv[row];
#pragma unroll
      for (int a = 0; a < 6; ++a) p += rr[1 + a] * yc[a];
      mpart += p * (rr[13] - p / 2.0);
    }
  };
  if (!kChunked) {
    model(nrows);
  } else {
    for (int r0 = 0; r0 < nrows; r0 += kChunkRows) {
      const int nr = min(kChunkRows, nrows - r0);
      __syncthreads();
      if (kEst) load_rows_q<true>(P, scale, yF, yf, c, o0, r0, nr, nrows, rows, qv, yl1, yl2, jrows_l);
      else load_rows_q(P, scale, yF, yf, c, o0, r0, nr, nrows, rows, qv);
      __syncthreads();
      model(nr);
    }
  }
  mpart = wave_sum(mpart);
  double st = 0.0, bad = 0.0;
  double *capc = v;   // (v is free again: the candidate capture pose, for the cost)
  if (lane < 6) {
    const double yv = yc[lane];
    const double d = -yv * scale[sc + lane];
    const double xo = x[sc + lane];
    const double xn = xo + d;
    xc[sc + lane] = xn;
    capc[lane] = xn;
    if (P.slot_free[sc + lane] && !direct) st = (xo - xn) * (xo - xn);   // (a direct group: counted on its f-block)
    bad = isfinite(yv) ? 0.0 : 1.0;
  }
  st = wave_sum(st);
  bad = wave_max(bad);
  if (lane == 0) {
    parts[(long)P_MODEL * P.nc + c] = mpart;
    parts[(long)P_STEP2 * P.nc + c] = st;
    parts[(long)P_YBAD * P.nc + c] = bad;
  }
  // the candidate's cost (k_cost fused): camera and tags of xc were written
  // by k_update_f, launched before this kernel
  if (with_cost) {
    __syncthreads();
    capture_cost<kChunked, kLoss, kSized, kDist>(P, xc, capc, c, parts);
  }
