// llt_levels.hip -- the level-launch executor of the reduced system's Cholesky
// (see llt_dag.hip for the storage, the plan and the persistent executor): one
// k_panel and one k_update launch per level of the plan, and the backward
// solve as one k_bs_gather / k_bs_solve pair per level.  The independent
// implementation the persistent executor is checked against bit for bit.
#include "llt_tile.h"

#include <algorithm>

namespace arslam {

namespace {

// Panel tasks of one level: task (i,k) factors the diagonal tile (k,k) (every
// task of column k does so redundantly, keeping the level to one launch) and
// either stores L_kk (i == k) or solves tile (i,k) against it.  L_kk goes to
// its own buffer Ld (64x64 per tile column), never over A_kk in S: the other
// tasks of the column may still be reading A_kk.
__global__ __launch_bounds__(256) void k_panel(double *__restrict__ S, const int *__restrict__ tid_map,
                                               int T, double *__restrict__ Ld,
                                               const int2 *__restrict__ tasks,
                                               int *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) double D[T64 * LQ];
  __shared__ __attribute__((aligned(16))) double X[T64 * LQ];
  __shared__ double inv[T64];
  __shared__ __attribute__((aligned(16))) double LTd[4 * 16 * LI];   // inverses of the 16x16 diagonal blocks
  __shared__ double colx[T64];
  __shared__ int bad;
  STAMP(0);
  if (*flag) return;
  const int tid = threadIdx.x;
  const int2 t = tasks[blockIdx.x];
  const int ti = t.x, k = t.y;
  const double *dk = tile_ptr(S, tid_map, T, k, k);
  double *xt = tile_ptr(S, tid_map, T, ti, k);
  load_tile_wg(dk, T64, D, tid);
  if (ti != k) load_tile_wg(xt, T64, X, tid);
  __syncthreads();
  STAMP(1);
  const bool ok = blocked_potrf64(D, inv, LTd, &bad, tid, colx);
  if (!ok) {
    if (ti == k && tid == 0) {
      int first = 0;
      while (first < T64 && D[first * LQ + first] > 0.0) ++first;
      atomicCAS(flag, 0, 1 + k * T64 + first);
    }
    return;
  }
  if (ti == k) {
    // L_kk, and its inverse (for the backward solve) while the column's
    // other tasks run their TRSMs
    store_tile_wg(Ld + (long)k * T64 * T64, T64, D, tid, true);
    blocked_trinv64(D, LTd, X, tid);
    __syncthreads();
    double *Xg = Ld + ((long)T + k) * T64 * T64;
#pragma unroll 4
    for (int m = 0; m < 16; ++m) {
      const int e = m * 256 + tid, r = e >> 6, c = e & 63;
      Xg[e] = (r >= c) ? X[c * LQ + r] : 0.0;
    }
    return;
  }
  STAMP(2);
  blocked_trsm64(X, D, inv, LTd, tid);
  STAMP(3);
  store_tile_wg(xt, T64, X, tid, false);
  STAMP(4);
}

// Update items of one level: tile (i,j) -= sum over the item's columns k of
// L_ik L_jk^T.  An unsplit target is one item (one workgroup writes the
// tile); a split target's chunks each store their partial product to a slot
// of `part`, and the chunk that arrives last sums the partials in chunk order
// and writes the tile (agent-scope release / acquire hand-off: correct for
// any placement of the chunks over XCDs).  4 waves x 32x32 on
// v_mfma_f64_16x16x4_f64, K = 64 per column; the next column's operand
// tiles are in flight while the current column's MFMAs run.
__global__ __launch_bounds__(256) void k_update(double *__restrict__ S, const int *__restrict__ tid_map,
                                                int T, const int2 *__restrict__ targets,
                                                const int4 *__restrict__ items,
                                                const int *__restrict__ ks,
                                                const int2 *__restrict__ split,
                                                double *__restrict__ part, int *__restrict__ cnt,
                                                const int *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) double sA[T64 * LM + 2];
  __shared__ __attribute__((aligned(16))) double sB[T64 * LM];
  if (*flag) return;
  const int4 it = items[blockIdx.x];
  const int2 pr = targets[it.x];
  const int ti = pr.x, tj = pr.y;
  const int q0 = it.y, q1 = it.z, sid = it.w;   // sid < 0: unsplit target
  const int tid = threadIdx.x;
  const int w = tid >> 6, lane = tid & 63;
  const int r0 = (w >> 1) * 32, c0 = (w & 1) * 32;
  const int li = lane & 15, lk = lane >> 4;
  dbl4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  dbl2 va[8], vb[8];
  auto fetch = [&](int q) {
    const int k = ks[q];
    const double *Ai = tile_ptr(S, tid_map, T, ti, k);
    const double *Bj = tile_ptr(S, tid_map, T, tj, k);
#pragma unroll
    for (int e8 = 0; e8 < 8; ++e8) {
      const int e = e8 * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
      va[e8] = *reinterpret_cast<const dbl2 *>(Ai + r * T64 + c2);
      vb[e8] = *reinterpret_cast<const dbl2 *>(Bj + r * T64 + c2);
    }
  };
  if (q0 < q1) fetch(q0);
  for (int q = q0; q < q1; ++q) {
    if (q > q0) __syncthreads();   // previous column's fragments consumed
#pragma unroll
    for (int e8 = 0; e8 < 8; ++e8) {
      const int e = e8 * 256 + tid, r = e >> 5, c2 = (e & 31) * 2;
      *reinterpret_cast<dbl2 *>(&sA[r * LM + c2]) = va[e8];
      *reinterpret_cast<dbl2 *>(&sB[r * LM + c2]) = vb[e8];
    }
    __syncthreads();
    if (q + 1 < q1) fetch(q + 1);
    // (gemm64_nt and, below, acc_pos written out: calling the shared helpers here
    // gives the same arithmetic but reallocates the kernel -- profiles/llt_split)
#pragma unroll 4
    for (int kk = 0; kk < T64 / 4; ++kk) {
      const int kc = kk * 4 + lk;
      const double a0 = sA[(r0 + li) * LM + kc];
      const double a1 = sA[(r0 + 16 + li) * LM + kc];
      const double b0 = sB[(c0 + li) * LM + kc];
      const double b1 = sB[(c0 + 16 + li) * LM + kc];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[3], 0, 0, 0);
    }
  }
  if (sid >= 0) {
    // split target (sid = split id << 8 | chunk): publish this chunk's partial
    // (fragment order, lane-contiguous 16-B stores), draw a ticket; the last
    // arriver sums every chunk's partial in chunk order
    const int2 sp = split[sid >> 8];   // {n_chunks, first slot}
    dbl2 *mine = reinterpret_cast<dbl2 *>(part + (long)(sp.y + (sid & 255)) * 4096);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      mine[(2 * q) * 256 + tid] = dbl2{acc[q][0], acc[q][1]};
      mine[(2 * q + 1) * 256 + tid] = dbl2{acc[q][2], acc[q][3]};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int *is_last = reinterpret_cast<int *>(&sA[T64 * LM]);
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int old = __hip_atomic_fetch_add(cnt + (sid >> 8), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *is_last = old == sp.x - 1;
      if (old == sp.x - 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    __syncthreads();
    if (!*is_last) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = dbl4{0, 0, 0, 0};
    for (int c = 0; c < sp.x; ++c) {
      const dbl2 *pc = reinterpret_cast<const dbl2 *>(part + (long)(sp.y + c) * 4096);
      dbl2 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = pc[u * 256 + tid];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[q][0] += v[2 * q].x;
        acc[q][1] += v[2 * q].y;
        acc[q][2] += v[2 * q + 1].x;
        acc[q][3] += v[2 * q + 1].y;
      }
    }
  }
  // f64 MFMA C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
  double *C = tile_ptr(S, tid_map, T, ti, tj);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int rb = r0 + (q >> 1) * 16, cb = c0 + (q & 1) * 16;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = rb + lk + 4 * reg, col = cb + li;
      C[row * T64 + col] -= acc[q][reg];
    }
  }
}

// z[j] = L[nR][j], the forward-substituted right-hand side: from S for the
// tiles left of the rhs row's own tile, from that tile's diagonal factor in Ld.
__global__ void k_init_z(const double *__restrict__ S, const int *__restrict__ tid_map, int T,
                         const double *__restrict__ Ld, long nR, long N, double *__restrict__ z) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const long kr = nR / T64;
  double v = 0.0;
  if (j < nR) {
    if (j >= kr * T64) v = Ld[kr * T64 * T64 + (nR - kr * T64) * T64 + (j - kr * T64)];
    else v = tile_ptr(S, tid_map, T, (int)kr, (int)(j / T64))[(nR - kr * T64) * T64 + (j % T64)];
  }
  z[j] = v;
}

// Backward solve L^T y = z, level by level from the root.  For a level:
//   k_bs_gather: one workgroup per gathered tile (i,k) (i > k, an ancestor
//     already solved): part_g = L_ik^T y_i, stored to its own slot;
//   k_bs_solve:  one workgroup per column k: sums its gathers' partials in
//     the plan's order reversed (deterministic: every rank of a sharded solve
//     computes the same bits; k_bsolve_dag's order), then solves L_kk^T y_k = z_k - sum (lane r owns row r,
//     16-row blocks, scalar broadcasts of y).
__global__ __launch_bounds__(256) void k_bs_gather(const double *__restrict__ S,
                                                   const int *__restrict__ tid_map, int T, long nR,
                                                   const int2 *__restrict__ tasks,
                                                   const double *__restrict__ yF,
                                                   double *__restrict__ part_out,
                                                   const int *__restrict__ flag) {
  __shared__ double part[4][T64];
  if (*flag) return;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int2 t = tasks[blockIdx.x];
  const long ri = (long)t.x * T64;
  const double *Lik = tile_ptr(S, tid_map, T, t.x, t.y);
  // (wave w: rows w, w + 4, ... into one accumulator, then the four waves'
  // sums left to right -- k_bsolve_dag's order, so the two executors give the
  // same bits of y)
  double a = 0.0;
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const int r = w + 4 * m;
    const double y = (ri + r < nR) ? yF[ri + r] : 0.0;
    a += Lik[r * T64 + lane] * y;
  }
  part[w][lane] = a;
  __syncthreads();
  if (w == 0) part_out[(long)blockIdx.x * T64 + lane] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// y_k = L_kk^{-T} (z_k - sum of the column's gathered partials), with the
// inverse X_kk from the panel: y[c] = sum_r X[r][c] acc[r] (4 waves x 16 rows,
// fixed-order combine).  Rows past nR carry acc = 0 and y = 0.
__global__ __launch_bounds__(256) void k_bs_solve(const double *__restrict__ Xinv, long nR,
                                                  const int *__restrict__ cols,
                                                  const int *__restrict__ gbeg,
                                                  const double *__restrict__ z,
                                                  const double *__restrict__ part,
                                                  double *__restrict__ yF,
                                                  const int *__restrict__ flag) {
  __shared__ double accs[T64];
  __shared__ double red[4][T64];
  if (*flag) return;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int k = cols[blockIdx.x];
  const long row0 = (long)k * T64;
  if (w == 0) {
    double acc = 0.0;
    const int ga = gbeg[blockIdx.x], gb = gbeg[blockIdx.x + 1];
    // 8 loads in flight, summed from the end of the plan's list to its start:
    // the nearest ancestor last, as k_bsolve_dag sums them
    for (int g = gb - 1; g >= ga; g -= 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(long)max(g - u, ga) * T64 + lane];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += (g - u >= ga) ? v[u] : 0.0;
    }
    accs[lane] = (row0 + lane < nR) ? z[row0 + lane] - acc : 0.0;
  }
  __syncthreads();
  const double *X = Xinv + (long)k * T64 * T64;
  double s = 0.0;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int r = 16 * w + rr;
    s += X[r * T64 + lane] * accs[r];
  }
  red[w][lane] = s;
  __syncthreads();
  if (w == 0 && row0 + lane < nR) yF[row0 + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

}  // namespace

void launch_dense_llt(const LltPlan &P, double *S, int *flag, hipStream_t s, LaunchTiming *timing) {
  if (P.n_split) (void)hipMemsetAsync(P.upd_cnt, 0, P.n_split * sizeof(int), s);
  for (int l = 0; l < P.nlev; ++l) {
    const int np = P.h_panel_off[l + 1] - P.h_panel_off[l];
    hipLaunchKernelGGL(k_panel, dim3((unsigned)np), dim3(256), 0, s, S, P.tile_id, P.T, P.ldiag,
                       P.panel + P.h_panel_off[l], flag);
    const int ni = P.h_item_off[l + 1] - P.h_item_off[l];
    if (ni > 0) {
      const bool rec = timing && timing->used < timing->cap;
      if (rec) (void)hipEventRecord(timing->ev[2 * timing->used], s);
      hipLaunchKernelGGL(k_update, dim3((unsigned)ni), dim3(256), 0, s, S, P.tile_id, P.T, P.upd_targets,
                         P.upd_items + P.h_item_off[l], P.upd_ks, P.upd_split, P.upd_part, P.upd_cnt, flag);
      if (rec) {
        (void)hipEventRecord(timing->ev[2 * timing->used + 1], s);
        timing->used++;
        timing->flops += P.h_upd_flops[l];
      }
    }
  }
}

void launch_dense_back_solve(const LltPlan &P, const double *S, long nR, double *z, double *yF,
                             const int *flag, hipStream_t s) {
  const long N = (long)P.T * T64;
  hipLaunchKernelGGL(k_init_z, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, S, P.tile_id, P.T, P.ldiag,
                     nR, N, z);
  for (int l = 0; l < P.nlev; ++l) {
    const int g0 = P.h_bsg_off[l], ng = P.h_bsg_off[l + 1] - g0;
    if (ng > 0)
      hipLaunchKernelGGL(k_bs_gather, dim3((unsigned)ng), dim3(256), 0, s, S, P.tile_id, P.T, nR, P.bs_gather + g0, yF,
                         P.bs_part + (long)g0 * T64, flag);
    const int b0 = P.h_bs_off[l], nc = P.h_bs_off[l + 1] - b0;
    hipLaunchKernelGGL(k_bs_solve, dim3((unsigned)nc), dim3(256), 0, s, P.ldiag + (long)P.T * T64 * T64, nR,
                       P.bs_cols + b0,
                       P.bs_gbeg + b0, z, P.bs_part, yF, flag);
  }
}

}  // namespace arslam
