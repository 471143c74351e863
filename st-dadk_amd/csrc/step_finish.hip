// See step_finish.h.  A heterogeneous kernel in the manner of dw_all_kernel: the two kinds of workgroup are independent
// (the reduce jobs read the step's slabs and column partials, the knot tiles the per-knot sums of the gather), have
// the same shape (256 threads) and are each far too small to fill the chip, so one launch + drain is saved and
// nothing is lost.
#include "step_finish.h"
#include "gemm_body.h"
#include "knot_finish_body.h"

namespace stdadk {

__global__ __launch_bounds__(256) void step_finish_kernel(ReduceGroup grp, KnotFinishArgs a,
                                                          float *__restrict__ knot_parts, int n_knot_wg,
                                                          int *__restrict__ step_inc) {
  __shared__ float smem[3 * 4 * 64];   // the reduce body's 4 x 64 floats, or a knot tile's 3 x 4 x 64 partial sums
  __shared__ float red[4];
  if (blockIdx.x == 0 && threadIdx.x == 0 && step_inc) step_inc[0] += 1;   // nobody else touches it here
  const int nrb = grp.n_reduce_blocks;
  if ((int)blockIdx.x < nrb) {
    // reduce_jobs_kernel's workgroup, partial included: same sums in the same order
    const float sq = reduce_job_block(grp, (int)blockIdx.x, smem);
    if (grp.sq_parts) {              // workgroup-uniform
      const float s = wave_sum(sq);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
      __syncthreads();
      if (threadIdx.x == 0) grp.sq_parts[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    return;
  }
  // knot workgroup w: tiles w, w + n_knot_wg, ... (one tile each up to 64 * STDADK_SUMSQ_PARTS knots), ONE partial
  const int w = (int)blockIdx.x - nrb;
  const int n_tiles = (a.Ks + 63) / 64;
  float(*part)[4][64] = reinterpret_cast<float(*)[4][64]>(smem);
  float sq = 0.f;
  for (int tile = w; tile < n_tiles; tile += n_knot_wg) {     // workgroup-uniform
    if (tile != w) __syncthreads();                           // the previous tile's readers of `part` and `red`
    sq += knot_finish_tile(a, tile, part, red);
  }
  if (knot_parts) {
    const float s = wave_sum(sq);
    __syncthreads();                                          // the last tile's readers of `red`
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      knot_parts[w] = (red[0] + red[1]) + (red[2] + red[3]);
      for (int i = w + n_knot_wg; i < STDADK_SUMSQ_PARTS; i += n_knot_wg) knot_parts[i] = 0.f;
    }
  }
}

int step_finish_knot_blocks(int Ks) {
  const int64_t tiles = ceil_div(Ks, 64);
  return (int)(tiles < STDADK_SUMSQ_PARTS ? tiles : STDADK_SUMSQ_PARTS);
}

int launch_step_finish(ReduceGroup &grp, const KnotFinishArgs &a, float *knot_parts, int *step_inc, hipStream_t st) {
  STDADK_REQUIRE(!grp.sq_region_parts && !grp.step_inc, STDADK_E_ARG,
                 "step_finish: the region partials and the step counter of a reduce table do not ride here");
  STDADK_REQUIRE(a.Ks > 0 && a.part && a.centers && a.d_centers && a.d_log_bw, STDADK_E_ARG,
                 "step_finish: no knots / NULL pointer");
  const int nrb = reduce_jobs_block_count(grp);
  const int nk = step_finish_knot_blocks(a.Ks);
  STDADK_LAUNCH(step_finish_kernel, dim3((unsigned)(nrb + nk)), dim3(256), 0, st, grp, a, knot_parts, nk, step_inc);
  STDADK_CHECK_LAUNCH("step_finish");
  return 0;
}

}  // namespace stdadk
