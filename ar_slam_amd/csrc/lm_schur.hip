// lm_schur.hip -- the Schur elimination of the LM step and the assembly of
// the reduced system (fp64, gfx950).
//
// k_schur, one wavefront per capture (the eliminated e-block): from the rows
// k_linearize stored, the wave forms the capture's normal-equation blocks on
// MFMA (lane (lk, li) of an observation's Gram matrix holds G[lk + 4 reg][li])
//   U_c = E'E + D_c^2 (6x6), W_c = E'F (6 x (1 + 6 n_tags)), F'F, E'r, F'r
// and writes its Schur contribution F'F - W'U^{-1}W (lower block triangle)
// and F'r - W'U^{-1}E'r to its block-packed slab slot; its blocks past the
// captures clear S and reset the Cholesky executors.  k_schur_gather, one
// wave per destination block (lane -> element and lane group, GatherLane),
// sums the slab blocks of each destination in capture order into the compact
// tiles of the reduced system, k_schur_combine the pieces of a split
// destination in piece order; k_prep_reduced (or the gather itself, prep
// mode) adds D_f^2 and sets the padding and rhs rows' diagonal.
//
// Every sum is fixed-order (no atomics in any of them), so the reduced system
// is bit-identical run to run.
#include "lm_launch.h"
#include "lm_rows.h"
#include "schur_store_table.h"

#include "arslam_lm.h"

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

namespace arslam {

#ifdef ARSLAM_SCHUR_STAMPS
__device__ unsigned long long g_schur_ph[16];
#define SCHUR_STAMP_INIT unsigned long long _st0 = clock64()
#define SCHUR_STAMP(k)                                                         \
  do {                                                                         \
    const unsigned long long _n = clock64();                                   \
    if (threadIdx.x == 0) atomicAdd(&g_schur_ph[k], _n - _st0);                \
    _st0 = _n;                                                                 \
  } while (0)
void debug_read_schur_stamps(unsigned long long *out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_schur_ph), sizeof(g_schur_ph));
}
#else
#define SCHUR_STAMP_INIT do {} while (0)
#define SCHUR_STAMP(k) do {} while (0)
void debug_read_schur_stamps(unsigned long long *out) {
  for (int i = 0; i < 16; ++i) out[i] = 0;
}
#endif

namespace {

// k_schur<false>'s output-stage descriptors: a constant of the code object
__device__ const SchurStoreTable g_schur_store = make_schur_store_table();

// A direct group of the mixed e-set (MixedProblem): residuals whose two poses
// are both on the reduced side, grouped by their capture, whose pose is the
// group's last local f-block (nblk - 1: no residual lists it, so its W, F'r and
// F'F entries stayed zero).  Nothing is eliminated: the stored local system is
// the plain normal-equation blocks of [f | tag blocks | own pose | r] (Ceres'
// SchurEliminator adds such rows to the reduced system as they are), the own
// pose's from the capture-wide sums U = E'E, E'f, E'F_u and E'r.
__device__ void store_direct_group(double *out, int nblk, int m, const double *U, const double *Etr, const double *W,
                                   const double *Ftr, const double *FF, double ff00, int lane) {
  const int own = nblk - 1;
  // local column x: 0 f, 1 a tag block's row, 2 the own pose's, 3 the rhs; u its block, i the row in it
  auto cls = [&](int x, int &u, int &i) {
    u = x >= 1 && x < m ? (x - 1) / 6 : 0;
    i = x >= 1 && x < m ? (x - 1) - 6 * u : 0;
    return x == 0 ? 0 : x == m ? 3 : (u == own ? 2 : 1);
  };
  for (int Ub = 0; Ub <= nblk + 1; ++Ub) {
    const int sU = schur_blk_size(Ub, nblk), p0 = schur_blk_start(Ub, nblk), ncol = p0 + sU;
    double *dst = out + schur_block_off(Ub, 0, nblk);
    for (int e = lane; e < sU * ncol; e += kWave) {
      const int ip = e / ncol, q = e - ip * ncol, p = p0 + ip;
      int ua, ia, ub, ib;
      int ka = cls(q, ua, ia), kb = cls(p, ub, ib);   // (the pair in f < tag < own < rhs order)
      if (ka > kb || (ka == kb && q > p)) {
        const int tk = ka, tu = ua, ti = ia;
        ka = kb; ua = ub; ia = ib;
        kb = tk; ub = tu; ib = ti;
      }
      double v = 0.0;
      if (ka == 0) {
        v = kb == 0 ? ff00 : kb == 1 ? FF[28 * ub + 21 + ib] : kb == 2 ? W[ib * m] : Ftr[0];
      } else if (ka == 1) {
        if (kb == 1) {
          if (ua == ub) {
            const int lo = min(ia, ib), hi = max(ia, ib);
            v = FF[28 * ua + lo * 6 - lo * (lo - 1) / 2 + (hi - lo)];
          }
        } else {
          v = kb == 2 ? W[ib * m + 1 + 6 * ua + ia] : Ftr[1 + 6 * ua + ia];
        }
      } else if (ka == 2) {
        v = kb == 2 ? U[6 * ia + ib] : Etr[ia];
      }
      const int V = schur_blk(q, m), q0V = schur_blk_start(V, nblk);
      dst[(long)sU * q0V + ip * schur_blk_size(V, nblk) + (q - q0V)] = v;
    }
  }
}

// Schur elimination of capture c (ComputeTrustRegionStep's DENSE_SCHUR
// eliminate step, one capture = one e-block; the normal-equation blocks from
// per-observation Gram matrices on MFMA): the packed local reduced system
//   [F'F - W' U^-1 W | F'r - W' U^-1 E'r],  U = E'E + D_c^2, W = E'F,
// over the local f-side columns (f, then 6 per distinct tag of the capture),
// stored for k_schur_gather.  One wave per capture.
// kBig = false: the main launch (captures of at most kSchurMfmaBlocks tags,
// the output as one MFMA product; the blocks past the captures clear S and
// reset the executors); true: the captures of more tags (cap_list), one block
// row of the output at a time.  Two instances, so the main one carries no
// registers for the other's path.
template <bool kBig>
__global__ __launch_bounds__(kWave) void k_schur(DevProblem P, const double *__restrict__ scale,
                                                 const double *__restrict__ diag, double radius,
                                                 double *__restrict__ zero_tiles, long n_zero, ExecReset er,
                                                 const int *__restrict__ cap_list) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  SCHUR_STAMP_INIT;
  // (cap_list: the second launch, over the captures with more than
  // kSchurMfmaBlocks distinct tags; the main launch then skips them)
  const int c = kBig ? cap_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
  if (c >= P.nc + n_zero) {
    // the blocks past the tiles: the persistent executors' reset (ExecReset;
    // launch_exec_reset's work when the LM diagonal needs no update)
    exec_reset_elem(er, (long)(c - P.nc - n_zero) * kWave + lane);
    return;
  }
  if (c >= P.nc) {
    // the blocks past the captures clear one 64x64 tile of S each (the gather
    // writes only the assembled blocks; the rest of S must be zero): the
    // stores overlap the latency-bound capture waves instead of a memset
    // launch of their own
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2 *z = reinterpret_cast<d2 *>(zero_tiles + (long)(c - P.nc) * 4096);
#pragma unroll 8
    for (int e = lane; e < 2048; e += kWave) z[e] = d2{0.0, 0.0};
    return;
  }
  const int o0 = P.cap_start[c], k = P.cap_start[c + 1] - o0;
  if (k == 0) return;
  const int nrows = 8 * k;
  const int b0 = P.cap_blk_start[c], nblk = P.cap_blk_start[c + 1] - b0;
  if (!kBig && nblk > kSchurMfmaBlocks) return;   // (the second launch's)
  const int m = 1 + 6 * nblk;   // local f-side columns: f, then 6 per distinct tag
  // LDS (schur_lds_bytes): no copy of the Jacobian rows (they go from HBM
  // straight into the MFMA operand registers), so ~8 KB per wave at 8 tags:
  // 4-5 waves per SIMD instead of the 2.75 the 13.5 KB row-staging layout
  // allowed (latency-bound kernel)
  const SchurLds lds = schur_lds(nblk);
  double *stage = sm;                    // 6 min(m + 1, 64): the MFMA product's Z operand
  double *tscale = sm + lds.tscale;      // 6 kObsChunk: the chunk's observations' tag column scales
  double *U = sm + lds.U;                // 36
  double *Ui = sm + lds.Ui;              // 36
  double *Etr = sm + lds.Etr;            // 8
  double *W = sm + lds.W;                // 6*m
  double *Ftr = sm + lds.Ftr;            // m (+pad)
  double *FF = sm + lds.FF;              // 28 per tag block: F_u'F_u (21, packed), F_0'F_u (6), pad
  int *lblk = (int *)(sm + lds.lblk);    // kObsChunk: the chunk's observations' tag blocks
  double *ff00 = sm + lds.ff00;          // F_0'F_0

  // the first eight observations' Jacobian rows (the Gram loop's operands
  // below) are loaded before the prologue's dependent loads (obs_tag -> the
  // tag scales), so the two latencies overlap
  const int li = lane & 15, lk = lane >> 4;
  const bool valid = li < 14;
  // (column li of the row is stored column jrow_col(li): lanes 7..9 read the
  // translation column lanes 1..3 read)
  const double *jb = P.jrows + 8L * o0 * kJStored + (long)jrow_col(min(li, 13)) * nrows;
  double jv[16];
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int st = 0; st < 2; ++st)
      jv[2 * u + st] = (valid && u < k) ? jb[8 * u + 4 * st + lk] : 0.0;
  static_assert(kObsChunk == 8, "k_schur's operand registers hold eight observations");
  // the tag scales and blocks of a chunk of kObsChunk observations (reloaded
  // beside the operand registers in the Gram loop)
  auto stage_chunk = [&](int q0) {
    const int kc = min(kObsChunk, k - q0);
    if (lane < kc) lblk[lane] = P.obs_lblk[o0 + q0 + lane];
    if (lane < 6 * kc) tscale[lane] = scale[slot_tag(P, P.obs_tag[o0 + q0 + lane / 6]) + lane % 6];
  };
  stage_chunk(0);
  __syncthreads();
  SCHUR_STAMP(0);
  // Every product below is an entry of an observation's Gram matrix over its
  // 8 rows and 14 columns [f | E (capture) | F (tag) | r]: G_q = R_q' R_q, two
  // v_mfma_f64_16x16x4_f64 per observation (columns padded to 16; lane
  // (lk, li) supplies row 4s + lk, column li as both operands; the result is
  // G_q[lk + 4 reg][li]).  The capture-wide sums (U = E'E, E'r, E'f, f'r, f'f)
  // add the observations' Grams in observation order; the per-tag-block
  // products (W_u = E'F_u, F_u'r, F_u'F_u, f'F_u) are added into LDS per
  // observation (a tag seen twice in one capture sums into one block).
  {
    for (int e = lane; e < 6 * m + m + (m & 1) + 28 * nblk; e += kWave) W[e] = 0.0;   // W, Ftr, FF: contiguous
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    typedef double dbl4v __attribute__((ext_vector_type(4)));
    dbl4v tot = {0, 0, 0, 0};
    // lane (lk, li) reads column li of rows 8q + lk and 8q + 4 + lk from the
    // capture's column-major Jacobian block (load_rows' layout), eight
    // observations' loads in flight at once, and scales it as load_rows does
    // (the same products: the Grams are bit-identical)
    const double *sc = scale + slot_cap(P, c);
    const double cs = li == 0 ? scale[0] : li <= 6 ? sc[li - 1] : 1.0;   // (tag columns: tscale)
    const bool tagcol = li >= 7 && li <= 12;
    // Where this lane's Gram entries G[lk + 4 reg][li] go, as an LDS index
    // (W, Ftr and FF are contiguous) plus a stride per tag block u: one LDS
    // add per register and observation instead of a divergent if-chain
    //   E'F_u  : W[(r-1) m + 1 + 6u + (c-7)]          r 1..6,  c 7..12
    //   F_u'r  : Ftr[1 + 6u + (r-7)]                    r 7..12, c 13
    //   F_u'F_u: FF[28u + a*6 - a(a-1)/2 + (b-a)]       r 7..12, r <= c <= 12
    //   f'F_u  : FF[28u + 21 + (c-7)]                   r 0,     c 7..12
    int acc_off[4], acc_stride[4];
    const int w_base = (int)(W - sm);
    {
      const int c = li, ftr0 = 6 * m, ff0 = ftr0 + m + (m & 1);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = lk + 4 * reg;
        int off = -1, st = 0;
        if (r >= 1 && r <= 6 && c >= 7 && c <= 12) { off = (r - 1) * m + 1 + (c - 7); st = 6; }
        else if (r >= 7 && r <= 12 && c == 13) { off = ftr0 + 1 + (r - 7); st = 6; }
        else if (r >= 7 && r <= 12 && c >= r && c <= 12) {
          const int a = r - 7, b = c - 7;
          off = ff0 + a * 6 - a * (a - 1) / 2 + (b - a); st = 28;
        } else if (r == 0 && c >= 7 && c <= 12) { off = ff0 + 21 + (c - 7); st = 28; }
        acc_off[reg] = off >= 0 ? w_base + off : 0;   // (no destination: stage[0], dead here)
        acc_stride[reg] = st;
      }
    }
    for (int q = 0; q < k; ++q) {
      if ((q & 7) == 0 && q > 0) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int st = 0; st < 2; ++st)
            jv[2 * u + st] = (valid && q + u < k) ? jb[8 * (q + u) + 4 * st + lk] : 0.0;
        stage_chunk(q);   // (the previous iteration ended at a wave barrier: its reads are done)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      dbl4v g = {0, 0, 0, 0};
      const double s = tagcol ? tscale[6 * (q & 7) + li - 7] : cs;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        double v = 0.0;
        switch (q & 7) {   // (register array: constant indices only)
          case 0: v = jv[0 + st]; break;
          case 1: v = jv[2 + st]; break;
          case 2: v = jv[4 + st]; break;
          case 3: v = jv[6 + st]; break;
          case 4: v = jv[8 + st]; break;
          case 5: v = jv[10 + st]; break;
          case 6: v = jv[12 + st]; break;
          default: v = jv[14 + st]; break;
        }
        v = li == 13 ? v : v * s;   // the residual column is not scaled
        g = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, g, 0, 0, 0);
      }
      tot += g;
      const int u = lblk[q & 7] - 1;   // the observation's tag block
      // this lane's entries G[lk + 4 reg][li] (acc_off above): the four
      // destinations are distinct, so their reads go out together
      int di[4];
      double dv[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        di[reg] = acc_off[reg] + acc_stride[reg] * u;
        dv[reg] = sm[di[reg]];
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sm[di[reg]] = dv[reg] + g[reg];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = lk + 4 * reg, c = li;
      const double v = tot[reg];
      if (r >= 1 && r <= 6 && c >= 1 && c <= 6) U[6 * (r - 1) + (c - 1)] = v;   // E'E
      else if (r >= 1 && r <= 6 && c == 13) Etr[r - 1] = v;                     // E'r
      else if (r >= 1 && r <= 6 && c == 0) W[(r - 1) * m] = v;                  // E'f
      else if (r == 0 && c == 13) Ftr[0] = v;                                   // f'r
      else if (r == 0 && c == 0) *ff00 = v;                                     // f'f
    }
  }
  __syncthreads();
  SCHUR_STAMP(1);
  if (group_direct(P, c)) {
    store_direct_group(P.slab + P.cap_off[c], nblk, m, U, Etr, W, Ftr, FF, *ff00, lane);
    return;
  }
  // (U + D_c^2)^{-1}: every lane factors U (one reciprocal per pivot), lane j
  // solves for column j
  {
    const long sc = slot_cap(P, c);
    double L[21];
    double rd[6];
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) L[e++] = U[6 * i + j] + (i == j ? lm_d2(diag, sc + i, radius) : 0.0);
#define LI6(i, j) L[(i) * ((i) + 1) / 2 + (j)]
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double d = LI6(j, j);
#pragma unroll
      for (int p = 0; p < j; ++p) d -= LI6(j, p) * LI6(j, p);
      const double sd = sqrt(d);
      rd[j] = 1.0 / sd;
      LI6(j, j) = sd;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double v = LI6(i, j);
#pragma unroll
        for (int p = 0; p < j; ++p) v -= LI6(i, p) * LI6(j, p);
        LI6(i, j) = v * rd[j];
      }
    }
    if (lane < 6) {
      double ev[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double v = (i == lane) ? 1.0 : 0.0;
#pragma unroll
        for (int p = 0; p < i; ++p) v -= LI6(i, p) * ev[p];
        ev[i] = v * rd[i];
      }
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double v = ev[i];
#pragma unroll
        for (int p = i + 1; p < 6; ++p) v -= LI6(p, i) * ev[p];
        ev[i] = v * rd[i];
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) Ui[6 * i + lane] = ev[i];
    }
#undef LI6
  }
  __syncthreads();
  if (lane < 36) P.cap_ui[36L * c + lane] = Ui[lane];   // reused by k_backsub
  SCHUR_STAMP(2);
  SCHUR_STAMP(3);
  // block-packed rows (row m is the rhs; entries of constant blocks are never
  // gathered; schur_block_off): lane q owns column q, z = (U + D_c^2)^{-1}
  // W[:, q] in registers; row p is wave-uniform, so its W column (the rhs
  // row: E'r) is an LDS broadcast.  One block row U at a time is staged in
  // LDS (over the dead Jacobian rows) in its final layout, then copied out
  // with contiguous stores.
  //   (p, q) = F_p'F_q - W_p' z_q,   (m, q) = F_q'r - (E'r)' z_q
  double *out = P.slab + P.cap_off[c];
  auto make_z = [&](int q, double z[6]) {
    if (q < m) {
      double wq[6];
#pragma unroll
      for (int b = 0; b < 6; ++b) wq[b] = W[b * m + q];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += Ui[6 * a + b] * wq[b];
        z[a] = s;
      }
    } else {
#pragma unroll
      for (int a = 0; a < 6; ++a) z[a] = 0.0;
    }
  };
  const bool one_chunk = !kBig;   // (m + 1 <= kWave)
  // the output stage's descriptors (schur_store_table.h), one 16-byte entry per
  // tile and lane: the first tile row's are fetched before z is formed
  typedef unsigned int u4v __attribute__((ext_vector_type(4)));
  const u4v *desc = reinterpret_cast<const u4v *>(&g_schur_store.e[one_chunk ? nblk - 1 : 0][0][lane][0]);
  u4v dsc[4];
  if (one_chunk) {
    dsc[0] = desc[0];
    dsc[1] = desc[kWave];
  }
  double z[6];
  if (one_chunk) make_z(lane, z);
  if (one_chunk) {
    // All M = m + 1 local rows at once as one MFMA product C = Wx' Z (K = 6,
    // padded to 8), Wx = [W | E'r] (6 x M), Z = [z_0 .. z_{m-1} | 0] (6 x M):
    // C[p][q] = W_p' z_q, the rhs row's (E'r)' z_q at p = m.  Only the 16x16
    // tiles that hold stored (lower block-triangle) entries are formed; each
    // lane then writes its entries F_p'F_q - C[p][q] (the F'F / F'r / f'f
    // terms where they are nonzero) straight to their block-packed slab slots.
    const int M = m + 1;
    const int li = lane & 15, lk = lane >> 4;
    double *Zs = stage;   // 6 M doubles: Zs[a M + q]
    if (lane < M)
#pragma unroll
      for (int a = 0; a < 6; ++a) Zs[a * M + lane] = z[a];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double Aop[4][2], Bop[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int a = 4 * kb + lk, pq = 16 * r + li;
        const bool in = a < 6 && pq < M;
        Aop[r][kb] = in ? (pq < m ? W[a * m + pq] : Etr[a]) : 0.0;
        Bop[r][kb] = in ? Zs[a * M + pq] : 0.0;
      }
    typedef double dbl4v __attribute__((ext_vector_type(4)));
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    // the capture's slab as a buffer: the stores below are range-checked
    // against it (c, nblk and the slab base are wave-uniform)
    const __amdgpu_buffer_rsrc_t slab_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(schur_slab_size(nblk) * sizeof(double)), 0x00020000);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (16 * r >= M) break;
      // the next tile row's descriptors are fetched beside this row's products
      // (the table holds all 13 tiles for every nblk: no bound to check)
      u4v dn[4];
      if (r < 3) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          if (cc <= r + 2) dn[cc] = desc[(schur_store_row_tile(r + 1) + cc) * kWave];
      }
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        if (cc > r + 1 || 16 * cc >= M) break;
        dbl4v acc = {0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Aop[r][0], Bop[cc][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Aop[r][1], Bop[cc][1], acc, 0, 0, 0);
        // element (16 r + lk + 4 reg, 16 cc + li): its F'F / F'r / f'F / f'f
        // term (a zero word where it has none) minus the product, to its slot
        // (a "not stored" entry's offset is past the slab: the store is dropped)
        double ff[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          ff[reg] = *reinterpret_cast<const double *>(
              reinterpret_cast<const char *>(sm) + ((dsc[cc][reg] >> kSchurStoreLdsShift) & kSchurStoreMask));
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, ff[reg] - acc[reg]), slab_rsrc,
                                                (int)(dsc[cc][reg] & kSchurStoreMask), 0, 0);
      }
      if (r < 3) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          if (cc <= r + 2) dsc[cc] = dn[cc];
      }
    }
  } else
  for (int U = 0; U <= nblk + 1; ++U) {
    // (more than kSchurMfmaBlocks tags: one block row U at a time, each entry
    // stored straight to its block-packed slot)
    const int sU = schur_blk_size(U, nblk), p0U = schur_blk_start(U, nblk), ncol = p0U + sU;
    double *dst = out + schur_block_off(U, 0, nblk);
    for (int q0 = 0; q0 < ncol; q0 += kWave) {
      const int q = q0 + lane;
      if (!one_chunk) make_z(q, z);
      const int V = schur_blk(min(q, m), m), sV = schur_blk_size(V, nblk), q0V = schur_blk_start(V, nblk);
      const int uq = V - 1, iq = q - q0V;   // tag block and row inside it (V in 1..nblk)
      if (sU == 6) {
        // a tag block row: the 36 W entries of its six rows read up front
        // (independent broadcasts), then six rows of six FMAs
        const int up = U - 1;
        double wv[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int a = 0; a < 6; ++a) wv[i][a] = W[a * m + p0U + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          double s = 0.0;
#pragma unroll
          for (int a = 0; a < 6; ++a) s += wv[i][a] * z[a];
          double ff = 0.0;
          if (q == 0) {
            ff = FF[28 * up + 21 + i];
          } else if (uq == up) {   // F_u'F_u packed upper (a <= b)
            const int lo = min(i, iq), hi = max(i, iq);
            ff = FF[28 * up + lo * 6 - lo * (lo - 1) / 2 + (hi - lo)];
          }
          if (q < ncol) dst[6 * q0V + i * sV + (q - q0V)] = ff - s;
        }
      } else {   // the f row (p = 0) or the rhs row (p = m)
        const int p = p0U;
        const double *wp = p < m ? W + p : Etr;
        const int st = p < m ? m : 1;
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) s += wp[a * st] * z[a];
        double ff = 0.0;
        if (p == m) ff = q < m ? Ftr[q] : 0.0;
        else ff = *ff00;   // p == 0: only q == 0 is stored
        if (q < ncol) dst[q0V + (q - q0V)] = ff - s;
      }
    }
  }
  SCHUR_STAMP(4);
}

// Destination block geometry: E = sX sY elements (1 row for f and the rhs,
// 6 for a tag), G = 64 / E lane groups; lane -> (element (i, j), group).
struct GatherLane {
  int E, G, el, grp, i, j;
  __device__ GatherLane(const DevProblem &P, int2 rr, int lane) {
    const int sx = (rr.x == P.nR || rr.x == P.cam_row) ? 1 : 6;
    const int sy = rr.y == P.cam_row ? 1 : 6;
    E = sx * sy;
    G = kWave / E;
    el = lane % E;
    grp = lane / E;
    i = el / sy;
    j = el % sy;
  }
};

// Lanes < E of the wave: the sum of the groups' partials, in group order.
__device__ __forceinline__ double gather_groups(double s, const GatherLane &g, double *part, int lane) {
  if (g.G == 1) return s;
  part[lane] = s;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double t = 0.0;
  if (lane < g.E)
    for (int q = 0; q < g.G; ++q) t += part[q * g.E + lane];
  return t;
}

// Sum of the captures' packed local systems into the reduced tiles: one wave
// per work item (a destination block (rX, rY), or a <= 64-contribution piece
// of one).  The wave stages the item's contribution descriptors in LDS; the
// G lane groups stride over them with 8 slab loads in flight per lane, and
// the groups' partials are added in group order -- a fixed summation order,
// no atomics.  Pieces store partial sums for k_schur_combine.
// The D_f^2 of a reduced row's diagonal element (prep: the gather adds it when
// it writes the element, k_prep_reduced's work), else 0.
__device__ __forceinline__ double prep_d2(const DevProblem &P, const double *diag, double radius, long r,
                                          long col) {
  if (!diag || r != col || r >= P.nR) return 0.0;
  const int slot = P.row_slot[r];
  return slot >= 0 ? lm_d2(diag, slot, radius) : 0.0;
}

// k_prep_reduced's diagonal elements that no gather item writes: alignment
// padding and the rows past the rhs become identity rows, the rhs row a pivot
// large enough to stay positive (in prep mode the gather leaves the rhs-rhs
// element to this), the camera's l1/l2 rows get their D_f^2
__device__ __forceinline__ void prep_pad_row(const DevProblem &P, const double *diag, double radius, double *S,
                                             long i) {
  if (i >= P.N) return;
  if (i < P.nR && P.row_slot[i] >= 0) {
    // the camera's l1, l2 rows (zero Jacobian columns, no Schur block): D_f^2 only
    if (P.cam_row >= 0 && i > P.cam_row && i <= P.cam_row + 2)
      *reduced_elem(S, P, i, i) = lm_d2(diag, P.row_slot[i], radius);
    return;
  }
  *reduced_elem(S, P, i, i) = i == P.nR ? 1e300 : 1.0;
}

__global__ __launch_bounds__(256) void k_schur_gather(DevProblem P, double *__restrict__ S,
                                                      const double *__restrict__ diag, double radius) {
  __shared__ double part[4][kWave];
  __shared__ SchurContrib cts[4][kWave];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_item_blocks = (P.n_items + 3) / 4;
  if (diag && (int)blockIdx.x >= n_item_blocks) {   // (prep) the rows no item writes
    prep_pad_row(P, diag, radius, S, (long)(blockIdx.x - n_item_blocks) * 256 + threadIdx.x);
    return;
  }
  const int it = blockIdx.x * 4 + w;
  if (it >= P.n_items) return;
  const int4 item = P.gather_items[it];
  const int2 rr = P.dest_row[item.x];
  const GatherLane g(P, rr, lane);
  const int nk = item.z - item.y;   // (gather_partition: <= 64, or <= 16 per lane group)
  const bool staged = nk <= kWave;
  if (staged && lane < nk) cts[w][lane] = P.contrib[item.y + lane];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double s = 0.0;
  // (a long item -- a 1- or 6-element block summing up to 16 contributions
  // per group -- reads its descriptors itself; the same order either way)
  auto sum = [&](const SchurContrib *src) __attribute__((always_inline)) {
    for (int t0 = g.grp; t0 < nk; t0 += 8 * g.G) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = min(t0 + u * g.G, nk - 1);   // clamped: always a valid address
        const SchurContrib ct = src[t];
        v[u] = P.slab[ct.off + (ct.tr ? g.j * ct.ld + g.i : g.i * ct.ld + g.j)];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) s += (t0 + u * g.G < nk) ? v[u] : 0.0;
    }
  };
  if (g.grp < g.G) {
    if (staged) sum(cts[w]);
    else sum(P.contrib + item.y);
  }
  s = gather_groups(s, g, part[w], lane);
  if (lane >= g.E) return;
  if (item.w >= 0) {
    P.gather_part[(long)item.w * 36 + lane] = s;
  } else {
    const long r = rr.x + g.i, col = rr.y + g.j;
    if (r >= col && !(diag && r == P.nR && col == P.nR)) *reduced_elem(S, P, r, col) = s + prep_d2(P, diag, radius, r, col);
  }
}

// Split destinations: the pieces' partial sums, in piece order.
__global__ __launch_bounds__(256) void k_schur_combine(DevProblem P, double *__restrict__ S,
                                                       const double *__restrict__ diag, double radius) {
  __shared__ double part[4][kWave];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sp = blockIdx.x * 4 + w;
  if (sp >= P.n_splits) return;
  const int4 split = P.gather_splits[sp];
  const int2 rr = P.dest_row[split.x];
  const GatherLane g(P, rr, lane);
  double s = 0.0;
  if (g.grp < g.G) {
    for (int t0 = g.grp; t0 < split.z; t0 += 8 * g.G) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = P.gather_part[(long)(split.y + min(t0 + u * g.G, split.z - 1)) * 36 + g.el];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += (t0 + u * g.G < split.z) ? v[u] : 0.0;
    }
  }
  s = gather_groups(s, g, part[w], lane);
  const long r = rr.x + g.i, col = rr.y + g.j;
  if (lane < g.E && r >= col && !(diag && r == P.nR && col == P.nR))
    *reduced_elem(S, P, r, col) = s + prep_d2(P, diag, radius, r, col);
}

// S[i][i] += D_f^2 for the reduced (tag + camera) rows; alignment padding and
// the rows past the rhs become identity rows; the rhs row gets a pivot large
// enough to stay positive (its factor row is L^{-1} b, its pivot unused).
__global__ void k_prep_reduced(DevProblem P, const double *__restrict__ diag, double radius,
                               double *__restrict__ S, int which) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.N) return;
  if (which >= 0 && P.tile_class[i >> 6] != which) return;
  double *d = reduced_elem(S, P, i, i);
  if (i < P.nR) {
    const int slot = P.row_slot[i];
    if (slot >= 0) *d += lm_d2(diag, slot, radius);
    else *d = 1.0;
  } else if (i == P.nR) {
    *d = 1e300;
  } else {
    *d = 1.0;
  }
}

// test hook: S[row,row] = v after the LM diagonal was added (a forced
// indefinite reduced system, arslam_lm_debug_force_indefinite)
__global__ void k_debug_set_diag(DevProblem P, double *S, long row, double v) {
  if (threadIdx.x == 0) *reduced_elem(S, P, row, row) = v;
}

}  // namespace

// k_schur<true>'s dynamic-LDS limit on the current device, once per device
// (the attribute is per device; several host threads may reach it at once): a
// failure is an error, not a launch that later fails for its LDS size.  Called
// where the device is made current (ensure_stream), not per launch.
void set_schur_big_lds_attribute() {
  static std::mutex m;
  static std::vector<char> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) throw ApiError(ARSLAM_E_HIP, "hipGetDevice");
  std::lock_guard<std::mutex> g(m);
  if ((int)done.size() <= dev) done.resize(dev + 1, 0);
  if (done[dev]) return;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_schur<true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)schur_lds_bytes(kMaxSchurBlocks));
  if (e != hipSuccess)
    throw ApiError(ARSLAM_E_HIP, std::string("hipFuncSetAttribute(k_schur, dynamic LDS): ") + hipGetErrorString(e));
  done[dev] = 1;
}

void launch_schur(const DevProblem &P, const double *x, const double *scale, const double *diag,
                  double radius, double *S, hipStream_t s, bool prep, long zero_tiles, const ExecReset *er) {
  const ExecReset r = er ? *er : ExecReset{};
  if (P.nc == 0) {
    if (zero_tiles) (void)hipMemsetAsync(S, 0, (size_t)zero_tiles * 4096 * sizeof(double), s);
    if (prep) launch_prep_reduced(P, diag, radius, S, s);
    return;
  }
  // the main launch: captures of at most kSchurMfmaBlocks distinct tags (and
  // the tile clears and the executor reset); a second one, its LDS sized for
  // them, takes the captures with more
  const size_t lds = schur_lds_bytes(std::min(P.max_blk_per_cap, kSchurMfmaBlocks));
  const long reset_blocks = (r.n() + kWave - 1) / kWave;
  hipLaunchKernelGGL(k_schur<false>, dim3((unsigned)(P.nc + zero_tiles + reset_blocks)), dim3(kWave), lds, s, P, scale,
                     diag, radius, S, zero_tiles, r, (const int *)nullptr);
  if (P.n_big_caps > 0) {
    const size_t lds_big = schur_lds_bytes(P.max_blk_per_cap);
    // (dynamic LDS past 64 KiB: set once per device by the caller, ensure_stream)
    hipLaunchKernelGGL(k_schur<true>, dim3((unsigned)P.n_big_caps), dim3(kWave), lds_big, s, P, scale, diag, radius, S,
                       0L, ExecReset{}, P.big_caps);
  }
  const double *pd = prep ? diag : nullptr;
  const unsigned gb = (unsigned)((P.n_items + 3) / 4) + (prep ? (unsigned)((P.N + 255) / 256) : 0u);
  if (gb) hipLaunchKernelGGL(k_schur_gather, dim3(gb), dim3(256), 0, s, P, S, pd, radius);
  if (P.n_splits)
    hipLaunchKernelGGL(k_schur_combine, dim3((unsigned)((P.n_splits + 3) / 4)), dim3(256), 0, s, P, S, pd,
                       radius);
}

void launch_schur_gather(const DevProblem &P, const double *diag, double radius, double *S, hipStream_t s) {
  const unsigned gb = (unsigned)((P.n_items + 3) / 4) + (unsigned)((P.N + 255) / 256);
  hipLaunchKernelGGL(k_schur_gather, dim3(gb), dim3(256), 0, s, P, S, diag, radius);
  if (P.n_splits)
    hipLaunchKernelGGL(k_schur_combine, dim3((unsigned)((P.n_splits + 3) / 4)), dim3(256), 0, s, P, S, diag, radius);
}

void launch_prep_reduced(const DevProblem &P, const double *diag, double radius, double *S,
                         hipStream_t s, int which) {
  hipLaunchKernelGGL(k_prep_reduced, dim3((unsigned)((P.N + 255) / 256)), dim3(256), 0, s, P, diag,
                     radius, S, which);
}

void debug_set_reduced_diag(const DevProblem &P, double *S, long row, double v, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_set_diag, dim3(1), dim3(64), 0, s, P, S, row, v);
}

}  // namespace arslam
