// See step_finish.h.  A heterogeneous kernel in the manner of dw_all_kernel: the three kinds of workgroup are
// independent (the reduce jobs read the step's slabs and column partials, the knot tiles the per-knot sums of the
// gather, the head workgroup the output layer's column partials or its final gradient), have the same shape (256
// threads) and are each far too small to fill the chip, so a launch + drain per kind is saved and nothing is lost.
// No workgroup waits for another: what the head needs of the fixed-order sums it computes itself.
#include "step_finish.h"
#include "gemm_body.h"
#include "knot_finish_body.h"
#include "delta_body.h"

namespace stdadk {

// HEAD_NB blocks of a tall reduce job at once, b0 .. b0 + HEAD_NB - 1 (blocks past the job's end do nothing): per element
// the very operations of reduce_one_job_block's tall path in the same order -- a thread's every-16th partials in groups
// of 8 as (v0 + v2) + (v4 + v6) and (v1 + v3) + (v5 + v7), the rest one by one, s0 + s1 into LDS, the 16 sub-sums four
// at a time -- with the loads of the HEAD_NB blocks in flight together: one workgroup has to hide the latency that the
// reductions launch hides with as many workgroups as blocks.  smem: HEAD_NB * 256 floats; ends on a barrier.
constexpr int HEAD_NB = 8;
__device__ __forceinline__ void head_tall_blocks(const ReduceJob &jb, const int b0, float *smem) {
  constexpr int SG = 256 / REDUCE_TALL_COLS;
  float(*red)[SG][REDUCE_TALL_COLS] = reinterpret_cast<float(*)[SG][REDUCE_TALL_COLS]>(smem);
  const int tx = threadIdx.x % REDUCE_TALL_COLS, ty = threadIdx.x / REDUCE_TALL_COLS;
  float s0[HEAD_NB], s1[HEAD_NB];
  int c[HEAD_NB];
#pragma unroll
  for (int u = 0; u < HEAD_NB; ++u) { c[u] = (b0 + u) * REDUCE_TALL_COLS + tx; s0[u] = 0.f; s1[u] = 0.f; }
  int s = ty;
  for (; s + 7 * SG < jb.splits; s += 8 * SG) {
    float v[HEAD_NB][8];
#pragma unroll
    for (int u = 0; u < HEAD_NB; ++u)
#pragma unroll
      for (int k = 0; k < 8; ++k) v[u][k] = c[u] < jb.n ? jb.src[(int64_t)(s + SG * k) * jb.stride + c[u]] : 0.f;
#pragma unroll
    for (int u = 0; u < HEAD_NB; ++u)
      if (c[u] < jb.n) {
        s0[u] += (v[u][0] + v[u][2]) + (v[u][4] + v[u][6]);
        s1[u] += (v[u][1] + v[u][3]) + (v[u][5] + v[u][7]);
      }
  }
  for (; s < jb.splits; s += SG) {
#pragma unroll
    for (int u = 0; u < HEAD_NB; ++u)
      if (c[u] < jb.n) s0[u] += jb.src[(int64_t)s * jb.stride + c[u]];
  }
#pragma unroll
  for (int u = 0; u < HEAD_NB; ++u) red[u][ty][tx] = s0[u] + s1[u];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < HEAD_NB; ++u)
    if (ty == u && c[u] < jb.n) {
      float o = 0.f;
#pragma unroll
      for (int q = 0; q < SG; q += 4) o += (red[u][q][tx] + red[u][q + 1][tx]) + (red[u][q + 2][tx] + red[u][q + 3][tx]);
      jb.dst[c[u]] = o;
    }
  __syncthreads();
}

__global__ __launch_bounds__(256) void step_finish_kernel(ReduceGroup grp, KnotFinishArgs a,
                                                          float *__restrict__ knot_parts, int n_knot_wg,
                                                          int *__restrict__ step_inc, HeadFinishArgs h) {
  __shared__ float smem[3 * 4 * 64];   // the reduce body's 4 x 64 floats, or a knot tile's 3 x 4 x 64 partial sums; the head's
  __shared__ float head_red[HEAD_NB * 256];   // blocks in flight (head_tall_blocks)
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
  const int w = (int)blockIdx.x - nrb;
  if (w >= n_knot_wg) {
    // the head workgroup (the last of the launch, h.d_delta set).  Pending: the output layer's two fixed-order sums
    // first, HEAD_NB reduce workgroups' shares at a time; the barrier behind each group frees the shared buffer for the
    // next and makes what was written to dWo / dbo visible to the whole workgroup before the fold reads it
    __shared__ DeltaHeadShared sh;
    if (h.pending) {
      for (int j = 0; j < 2; ++j) {                  // (everything here is workgroup-uniform)
        if (h.job[j].wide) {
          for (int b = 0; b < h.nblk[j]; ++b) {
            reduce_one_job_block(h.job[j], b, smem);
            __syncthreads();
          }
        } else {
          for (int b = 0; b < h.nblk[j]; b += HEAD_NB) head_tall_blocks(h.job[j], b, head_red);
        }
      }
    } else if (h.zero_slots) {
      // a launch in front summed dWo / dbo among its other jobs: their squares are no part of the flat gradient's norm
      for (int i = threadIdx.x; i < h.n_zero; i += 256) h.zero_slots[i] = 0.f;
    }
    const float sq = delta_head_bwd_body<true>(h.delta, h.dWo, h.dbo, h.ldd, h.Q, h.d, h.lam_g, h.lam_l, h.d_delta,
                                               h.loss_sum, sh);
    if (h.sq_part) {
      const float t = block4_sum(sq, red);
      if (threadIdx.x == 0) h.sq_part[0] = t;
    }
    return;
  }
  // knot workgroup w: tiles w, w + n_knot_wg, ... (one tile each up to 64 * STDADK_SUMSQ_PARTS knots), ONE partial
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

// kernel arguments travel in the 4 KiB kernarg segment
static_assert(sizeof(ReduceGroup) + sizeof(KnotFinishArgs) + sizeof(HeadFinishArgs) + 64 <= 4096,
              "step_finish: kernel arguments exceed the kernarg segment");

int step_finish_knot_blocks(int Ks) {
  const int64_t tiles = ceil_div(Ks, 64);
  return (int)(tiles < STDADK_SUMSQ_PARTS ? tiles : STDADK_SUMSQ_PARTS);
}

// `wide` of a job outside a table, as reduce_jobs_block_count decides it; returns the job's workgroups
static int head_job_blocks(ReduceJob &jb) {
  ReduceGroup one;
  one.n = 1; one.job[0] = jb;
  const int nb = reduce_jobs_block_count(one);
  jb.wide = one.job[0].wide;
  return nb;
}

int launch_step_finish(ReduceGroup &grp, const KnotFinishArgs &a, float *knot_parts, int *step_inc, hipStream_t st,
                       const HeadFinishArgs *h_in) {
  STDADK_REQUIRE(!grp.sq_region_parts && !grp.step_inc, STDADK_E_ARG,
                 "step_finish: the region partials and the step counter of a reduce table do not ride here");
  const bool head = h_in && h_in->d_delta;
  STDADK_REQUIRE(head || a.Ks > 0, STDADK_E_ARG, "step_finish: neither knots nor a head to finish");
  STDADK_REQUIRE(a.Ks == 0 || (a.Ks > 0 && a.part && a.centers && a.d_centers && a.d_log_bw), STDADK_E_ARG,
                 "step_finish: no knots / NULL pointer");
  STDADK_REQUIRE(a.Ks > 0 || !knot_parts, STDADK_E_ARG, "step_finish: knot partials without knots");
  HeadFinishArgs h;
  if (head) {
    h = *h_in;
    STDADK_REQUIRE(h.delta && h.dWo && h.dbo && h.Q >= 2 && h.Q <= STDADK_MAX_Q && h.d >= 1 && h.ldd >= h.d + 1, STDADK_E_ARG,
                   "step_finish: head incomplete (Q=%d d=%d ldd=%lld)", h.Q, h.d, (long long)h.ldd);
    if (h.pending) {
      STDADK_REQUIRE(h.job[0].dst == h.dWo && h.job[1].dst == h.dbo && h.job[0].n == h.Q * h.d && h.job[1].n == h.Q, STDADK_E_ARG,
                     "step_finish: the head's reduce jobs do not write the output layer's gradient");
      for (int j = 0; j < 2; ++j) h.nblk[j] = head_job_blocks(h.job[j]);
    }
  }
  const int nrb = reduce_jobs_block_count(grp);
  const int nk = a.Ks > 0 ? step_finish_knot_blocks(a.Ks) : 0;
  STDADK_LAUNCH(step_finish_kernel, dim3((unsigned)(nrb + nk + (head ? 1 : 0))), dim3(256), 0, st, grp, a, knot_parts, nk,
                step_inc, h);
  STDADK_CHECK_LAUNCH("step_finish");
  return 0;
}

}  // namespace stdadk
