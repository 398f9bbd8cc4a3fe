// lm_schur_cam.hip -- the border of the Schur complement for the camera's l1, l2
// (the handle's "estimate the distortion" switch; fp64, gfx950).
//
// k_schur forms an e-block's contribution over its local columns [f | 6 per
// distinct tag]; its local system of m + 1 <= 64 rows and its store table are
// exactly full, so the two columns an estimated distortion adds do not enter
// it.  They are a border computed beside it: with the e-block's scaled rows
// [f | E | F | r] (jrows) and their l columns L_a (DevCamL::jrows_l), a in {l1, l2},
//   border(a, q) = L_a'F_q - (E'L_a)' (U + D_c^2)^-1 (E'F_q) = Lt_a'F_q,
//   Lt_a = L_a - E z_a,   z_a = (U + D_c^2)^-1 E'L_a,
// for every local column q (f, the tag columns, l_b with b <= a: F_q = L_b) and
// the rhs (F_q = r) -- the same projected column against all of them, so E'F_q
// is not formed again.  (U + D_c^2)^-1 is the cap_ui k_schur leaves for
// k_backsub.
//
// k_schur_cam, one wavefront per e-block after k_schur: lane l owns row l of a
// 64-row chunk, as in k_linearize and k_backsub.  The products are VALU, not
// MFMA: two columns against 13 would fill an eighth of a 16x16 tile.
// k_schur_cam_gather sums the e-blocks' borders into rows cam_row + 1 and
// cam_row + 2 of the compact tiles (and their rhs entries) after
// k_schur_gather, adding the rows' D_f^2.
//
// Every sum is fixed-order (no atomics): over an observation's 8 rows
// (obs_sum8), over a chunk's rows (wave_sum's tree), over the chunks and an
// e-block's observations in order, over the e-blocks in order or by a fixed
// thread assignment and tree.
#include "lm_launch.h"
#include "lm_rows.h"

namespace arslam {

namespace {

// LDS of k_schur_cam, in doubles: the chunk's per-observation tag sums
// [kObsChunk][12], the running sums of the local tag columns [nblk][12], and
// the chunk's observations' local blocks (kObsChunk ints)
__host__ __device__ constexpr int schur_cam_lds_doubles(int nblk) { return 12 * kObsChunk + 12 * nblk + kObsChunk / 2; }

__global__ __launch_bounds__(kWave) void k_schur_cam(DevProblem P, DevCamL CL, const double *__restrict__ scale) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int c = blockIdx.x, lane = threadIdx.x;
  const int o0 = P.cap_start[c], k = P.cap_start[c + 1] - o0;
  const int nblk = P.cap_blk_start[c + 1] - P.cap_blk_start[c];
  const int m = 1 + 6 * nblk, ld = m + 3;
  double *out = CL.cam_slab + cam_slab_off(P, c);
  if (k == 0) {   // (k_schur leaves no inverse for it; the capture-wide sums read every e-block's border)
    for (int e = lane; e < 2 * ld; e += kWave) out[e] = 0.0;
    return;
  }
  double *obsv = sm;                        // [kObsChunk][12]
  double *acc = obsv + 12 * kObsChunk;      // [nblk][12]: (u, a, j) at 12 u + 6 a + j
  int *lblk = (int *)(acc + 12 * nblk);     // [kObsChunk]
  const int nrows = 8 * k;
  const double *jb = P.jrows + 8L * o0 * kJStored;
  const double *lb = CL.jrows_l + 16L * o0;
  const double *sc = scale + slot_cap(P, c);
  const double sf = scale[0], sl0 = scale[1], sl1 = scale[2];
  double scv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) scv[i] = sc[i];

  // W_a = E'L_a: a wave sum per chunk and entry, the chunks in row order
  double W[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) W[e] = 0.0;
  for (int r0 = 0; r0 < nrows; r0 += kWave) {
    const int row = r0 + lane;
    const bool in = row < nrows;
    double E[6], L[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) E[i] = in ? jb[(long)(1 + i) * nrows + row] * scv[i] : 0.0;
    L[0] = in ? lb[row] * sl0 : 0.0;
    L[1] = in ? lb[nrows + row] * sl1 : 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 6; ++i) W[6 * a + i] += wave_sum(E[i] * L[a]);
  }
  // z_a = (U + D_c^2)^-1 W_a, the same in every lane
  double z[12];
  {
    const double *ui = P.cap_ui + 36L * c;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double u = ui[6 * i + j];
        s0 += u * W[j];
        s1 += u * W[6 + j];
      }
      z[i] = s0;
      z[6 + i] = s1;
    }
  }
  for (int e = lane; e < 12 * nblk; e += kWave) acc[e] = 0.0;
  // the capture-wide entries: (a, f) x2, (l1, l1), (l2, l1), (l2, l2), the rhs x2
  double tot[7];
#pragma unroll
  for (int e = 0; e < 7; ++e) tot[e] = 0.0;
  for (int r0 = 0; r0 < nrows; r0 += kWave) {
    const int row = r0 + lane;
    const bool in = row < nrows;
    const int kc = min(kObsChunk, k - (r0 >> 3));
    __syncthreads();   // (the previous chunk's reads of obsv and lblk are done; acc is cleared)
    if (lane < kc) lblk[lane] = P.obs_lblk[o0 + (r0 >> 3) + lane];
    const int t = in ? P.obs_tag[o0 + (row >> 3)] : 0;
    const double *st = scale + slot_tag(P, t);
    double E[6], F[6], L[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) E[i] = in ? jb[(long)(1 + i) * nrows + row] * scv[i] : 0.0;
    // (the tag's translation columns are the capture's, stored once: jrow_col)
#pragma unroll
    for (int j = 0; j < 6; ++j) F[j] = in ? jb[(long)jrow_col(7 + j) * nrows + row] * st[j] : 0.0;
    const double jf = in ? jb[row] * sf : 0.0;
    const double r = in ? jb[(long)jrow_col(13) * nrows + row] : 0.0;
    L[0] = in ? lb[row] * sl0 : 0.0;
    L[1] = in ? lb[nrows + row] * sl1 : 0.0;
    double Lt[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) s += E[i] * z[6 * a + i];
      Lt[a] = L[a] - s;
    }
    tot[0] += wave_sum(Lt[0] * jf);
    tot[1] += wave_sum(Lt[1] * jf);
    tot[2] += wave_sum(Lt[0] * L[0]);
    tot[3] += wave_sum(Lt[1] * L[0]);
    tot[4] += wave_sum(Lt[1] * L[1]);
    tot[5] += wave_sum(Lt[0] * r);
    tot[6] += wave_sum(Lt[1] * r);
    // per observation (8 consecutive lanes): Lt_a'F_j, then into its tag block in observation order
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double v = obs_sum8(Lt[a] * F[j]);
        if ((lane & 7) == 0) obsv[12 * (lane >> 3) + 6 * a + j] = v;
      }
    __syncthreads();
    for (int e = lane; e < 12 * nblk; e += kWave) {
      const int u = e / 12, aj = e - 12 * u;
      double s = acc[e];
      for (int q = 0; q < kc; ++q)
        if (lblk[q] - 1 == u) s += obsv[12 * q + aj];
      acc[e] = s;
    }
  }
  __syncthreads();
  for (int e = lane; e < 12 * nblk; e += kWave) {
    const int u = e / 12, aj = e - 12 * u, a = aj / 6, j = aj - 6 * a;
    out[a * ld + 1 + 6 * u + j] = acc[e];
  }
  if (lane == 0) {
    out[0] = tot[0];
    out[ld] = tot[1];
    out[m] = tot[2];
    out[m + 1] = 0.0;   // (l1, l2): the lower triangle holds (l2, l1)
    out[ld + m] = tot[3];
    out[ld + m + 1] = tot[4];
    out[m + 2] = tot[5];
    out[ld + m + 2] = tot[6];
  }
}

// Blocks 0..6: the capture-wide entries -- (l_a, f), (l_a, l_b), the rhs --
// each the sum over every e-block (e-block c in thread c mod 256, then one
// pairwise tree).  The blocks after them: one thread per (f-block t, a, j),
// the sum over the e-blocks that see t, in e-block order (camg_*).  Written
// into the compact tiles after k_schur_gather: the diagonal entries with their
// D_f^2 (prep_pad_row left D_f^2 alone there), constant f-blocks skipped.
__global__ __launch_bounds__(256) void k_schur_cam_gather(DevProblem P, DevCamL CL, double *__restrict__ S,
                                                          const double *__restrict__ diag, double radius) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const long r1 = P.cam_row + 1;
  if (blockIdx.x < 7) {
    const int d = blockIdx.x;
    // the entry's place in an e-block's border: row a, column f / m + b / m + 2
    const int a = d == 0 ? 0 : d == 1 ? 1 : d == 2 ? 0 : d <= 4 ? 1 : d - 5;
    const int colk = d <= 1 ? 0 : d == 2 ? 1 : d == 3 ? 1 : d == 4 ? 2 : 3;   // 0 f, 1 l1, 2 l2, 3 rhs
    double acc = 0.0;
    for (int c = t; c < P.nc; c += 256) {
      const int ld = cam_slab_ld(P, c), m = ld - 3;
      acc += CL.cam_slab[cam_slab_off(P, c) + (long)a * ld + (colk == 0 ? 0 : m + colk - 1)];
    }
    red[t] = acc;
    __syncthreads();
    for (int off = 128; off >= kWave; off >>= 1) {
      if (t < off) red[t] += red[t + off];
      __syncthreads();
    }
    if (t < kWave) {
      const double s = wave_tree_sum(red[t], kWave);
      if (t == 0) {
        if (colk == 0) *reduced_elem(S, P, r1 + a, P.cam_row) = s;
        else if (colk == 3) *reduced_elem(S, P, P.nR, r1 + a) = s;
        else *reduced_elem(S, P, r1 + a, r1 + colk - 1) = s + (colk - 1 == a ? lm_d2(diag, 1 + a, radius) : 0.0);
      }
    }
    return;
  }
  const long e = (long)(blockIdx.x - 7) * 256 + t;
  if (e >= 12L * P.nt) return;
  const int tt = (int)(e / 12), aj = (int)(e % 12), a = aj / 6, j = aj - 6 * a;
  const int tr = P.tag_row[tt];
  // (a free f-block no e-block sees has no border entry, and maybe no tile)
  if (tr < 0 || CL.camg_start[tt] == CL.camg_start[tt + 1]) return;
  double s = 0.0;
  for (int i = CL.camg_start[tt]; i < CL.camg_start[tt + 1]; ++i) {
    const int2 it = CL.camg_items[i];
    s += CL.cam_slab[cam_slab_off(P, it.x) + (long)a * cam_slab_ld(P, it.x) + 1 + 6 * it.y + j];
  }
  *reduced_elem(S, P, r1 + a, tr + j) = s;
}

// debug: reduced rows cam_row + b (b < 3) against every reduced column and the
// rhs, out of the compact tiles: out[b (nR + 1) + col], col = nR the rhs entry
// (the lower triangle holds (cam_row + b, col) for col <= cam_row + b; the rows'
// entries right of the diagonal are the later rows' and are returned mirrored)
__global__ void k_debug_cam_rows(DevProblem P, double *S, double *__restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * (P.nR + 1)) return;
  const long b = i / (P.nR + 1), col = i - b * (P.nR + 1), r = P.cam_row + b;
  // (a tile outside the factor's pattern: a structural zero)
  const auto at = [&](long rr, long cc) { return P.tile_id[(rr >> 6) * P.T + (cc >> 6)] < 0 ? 0.0 : *reduced_elem(S, P, rr, cc); };
  double v = 0.0;
  if (col == P.nR) v = at(P.nR, r);
  else if (col <= r) v = at(r, col);
  else if (col <= P.cam_row + 2) v = at(col, r);
  out[i] = v;
}

// debug: the whole padded reduced system out of the compact tiles, both
// triangles: out[i N + j] = element (max(i, j), min(i, j)) of the lower tiles,
// 0 where the factor has no tile.  A copy and nothing more.
__global__ void k_debug_reduced_dense(DevProblem P, const double *__restrict__ S, double *__restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P.N * P.N) return;
  const long i = e / P.N, j = e - i * P.N;
  const long r = i > j ? i : j, c = i > j ? j : i;
  const int id = P.tile_id[(r >> 6) * P.T + (c >> 6)];
  out[e] = id < 0 ? 0.0 : S[(long)id * 4096 + (r & 63) * 64 + (c & 63)];
}

}  // namespace

void launch_schur_cam(const DevProblem &P, const DevCamL &cl, const double *scale, const double *diag, double radius,
                      double *S, hipStream_t s) {
  if (P.nc == 0 || P.cam_row < 0) return;
  const size_t lds = sizeof(double) * schur_cam_lds_doubles(P.max_blk_per_cap);
  hipLaunchKernelGGL(k_schur_cam, dim3(P.nc), dim3(kWave), lds, s, P, cl, scale);
  launch_schur_cam_gather(P, cl, diag, radius, S, s);
}

void launch_schur_cam_gather(const DevProblem &P, const DevCamL &cl, const double *diag, double radius, double *S,
                             hipStream_t s) {
  if (P.nc == 0 || P.cam_row < 0) return;
  const unsigned tag_blocks = (unsigned)((12L * P.nt + 255) / 256);
  hipLaunchKernelGGL(k_schur_cam_gather, dim3(7 + tag_blocks), dim3(256), 0, s, P, cl, S, diag, radius);
}

void debug_cam_rows(const DevProblem &P, double *S, double *out, hipStream_t s) {
  const long n = 3 * (P.nR + 1);
  hipLaunchKernelGGL(k_debug_cam_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, S, out);
}

void debug_reduced_dense(const DevProblem &P, const double *S, double *out, hipStream_t s) {
  const long n = P.N * P.N;
  if (n == 0) return;
  hipLaunchKernelGGL(k_debug_reduced_dense, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, S, out);
}

}  // namespace arslam
