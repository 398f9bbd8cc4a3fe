// lm_exchange.hip -- the element-wise kernels around the multi-rank
// exchanges of lm_solve.hip (fp64, gfx950): the masks of what a rank holds
// (k_mask_y, k_own_copy), the packing of several arrays into one all-reduce
// buffer (k_pack, k_top_tail), and the all-gather of a few scalars through one
// SUM all-reduce (k_ag_put, k_ag_reduce).  One thread per element; the only
// sums, k_ag_reduce's, run in rank order, so every rank gets the same bits.
#include "lm_launch.h"

namespace arslam {

namespace {

// multi-rank y: the rows this rank solved (own subtree; the top rows on rank 0
// only, or on every rank with keep_top), every other row 0
__global__ void k_mask_y(DevProblem P, double *__restrict__ yF, int rank, int keep_top) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.nR) return;
  const int c = P.tile_class[i >> 6];
  if (!(c == 0 || (c == 1 && (rank == 0 || keep_top)))) yF[i] = 0.0;
}

__global__ void k_own_copy(DevProblem P, long first, long count, const double *__restrict__ src,
                           double *__restrict__ dst) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) dst[i] = P.f_own[first + i] ? src[i] : 0.0;
}

// Segments copied into (unpack = 0) or out of (1) one contiguous buffer, so
// several arrays cross the ranks in one all-reduce.
__global__ void k_pack(PackSegs sg, double *__restrict__ buf, int unpack) {
  long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (int q = 0; q < sg.n; ++q) {
    if (e < sg.len[q]) {
      if (unpack) sg.p[q][e] = buf[sg.off[q] + e];
      else buf[sg.off[q] + e] = sg.p[q][e];
      return;
    }
    e -= sg.len[q];
  }
}

__global__ void k_top_tail(const int *__restrict__ idx, int m, double *__restrict__ g, double *__restrict__ cn,
                           double *__restrict__ red, double *__restrict__ tail, int unpack) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * m + 2) return;
  double *v = e < m ? g + idx[e] : e < 2 * m ? cn + idx[e - m] : red + (e == 2 * m ? P_GF : P_CF);
  if (unpack) *v = tail[e];
  else tail[e] = *v;
}

// All-gather of a few scalars through one SUM all-reduce: this rank's fields
// (src[idx[f]]) into row `rank` of ag[nranks][kAgFields], every other row 0
// (x + 0 is exact, so the all-reduce hands every rank every rank's values)
__global__ void k_ag_put(const double *__restrict__ src, AgFields fl, double *__restrict__ ag, int nranks, int rank) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nranks * kAgFields) return;
  const int r = e / kAgFields, f = e % kAgFields;
  ag[e] = (r == rank && f < fl.n) ? src[fl.idx[f]] : 0.0;
}

// ... and their combination in rank order (sum, or max where fl.max bit f is
// set), the same bits on every rank, written back to dst[idx[f]]
__global__ void k_ag_reduce(const double *__restrict__ ag, AgFields fl, double *__restrict__ dst, int nranks,
                            HostOut ho) {
  const int f = threadIdx.x;
  if (f < fl.n) {
    const bool mx = (fl.max >> f) & 1u;
    double v = ag[f];
    for (int r = 1; r < nranks; ++r) {
      const double w = ag[r * kAgFields + f];
      v = mx ? fmax(v, w) : v + w;
    }
    dst[fl.idx[f]] = v;
  }
  if (!ho.seq_word) return;
  // the host's words (after every combined value: one block), fenced at
  // system scope, then the sequence number the host polls
  __syncthreads();
  for (int q = 0; q < ho.n; ++q)
    for (int e = f; e < ho.len[q]; e += blockDim.x) ho.dst[q][e] = ho.src[q][e];
  __threadfence_system();
  __syncthreads();
  if (f == 0) __hip_atomic_store(ho.seq_word, ho.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

void launch_mask_y(const DevProblem &P, double *yF, int rank, hipStream_t s, bool keep_top) {
  if (P.nR == 0) return;
  hipLaunchKernelGGL(k_mask_y, dim3((unsigned)((P.nR + 255) / 256)), dim3(256), 0, s, P, yF, rank, keep_top ? 1 : 0);
}

void launch_own_copy(const DevProblem &P, long first, long count, const double *src, double *dst, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_own_copy, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, P, first, count, src, dst);
}

void launch_pack(const PackSegs &sg, double *buf, bool unpack, hipStream_t s) {
  long tot = 0;
  for (int q = 0; q < sg.n; ++q) tot += sg.len[q];
  if (tot == 0) return;
  hipLaunchKernelGGL(k_pack, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, sg, buf, unpack ? 1 : 0);
}

void launch_top_tail(const int *idx, int m, double *g, double *cn, double *red, double *tail, bool unpack,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_top_tail, dim3((unsigned)((2 * m + 2 + 255) / 256)), dim3(256), 0, s, idx, m, g, cn, red, tail,
                     unpack ? 1 : 0);
}

void launch_ag_put(const double *src, const AgFields &fl, double *ag, int nranks, int rank, hipStream_t s) {
  hipLaunchKernelGGL(k_ag_put, dim3((unsigned)((nranks * kAgFields + 255) / 256)), dim3(256), 0, s, src, fl, ag,
                     nranks, rank);
}

void launch_ag_reduce(const double *ag, const AgFields &fl, double *dst, int nranks, hipStream_t s,
                      const HostOut *ho) {
  hipLaunchKernelGGL(k_ag_reduce, dim3(1), dim3(kAgFields), 0, s, ag, fl, dst, nranks, ho ? *ho : HostOut{});
}

}  // namespace arslam
