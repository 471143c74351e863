// The backward of the delta-reparameterised head as ONE 256-thread workgroup, shared by delta_head_bwd_kernel
// (loss.hip: stdadk_delta_head_backward_f32) and the head workgroup of step_finish_kernel (step_finish.hip: the
// one-call delta step): the same arithmetic in the same order, so the two paths give the same bits.
#pragma once
#include "common.h"

namespace stdadk {

struct DeltaHeadShared {
  float red[4];
  float wS[STDADK_MAX_Q];     // share of max(delta_k0, S_k) that flows into S_k
  float Psum;
};

// d_delta[k][j] = sum_{l>=k} (dbo | dWo)[l][j] + lam_g * dP_nc/d delta[k][j], j = 0..d; lam_l * P_nc into loss_sum.
// S_k by the 256-thread strided sum, wave_sum, then red[0..3] in order; the reverse cumulative sums from k = Q-1 down.
// The column loop strides by the workgroup: d + 1 may exceed 256.  SQ: returns the squares of the entries this thread
// wrote (else 0).  `sh` is free to overwrite on entry; the caller puts a barrier in front when something else used it.
// (dWo / dbo carry no __restrict__: the head workgroup may have written them itself, earlier in the same kernel)
template <bool SQ>
__device__ __forceinline__ float delta_head_bwd_body(const float *__restrict__ delta, const float *dWo,
                                                     const float *dbo, const int64_t ldd, const int Q,
                                                     const int d, const float lam_g, const float lam_l,
                                                     float *__restrict__ d_delta, float *__restrict__ loss_sum,
                                                     DeltaHeadShared &sh) {
  float *red = sh.red, *wS = sh.wS;
  const int tid = threadIdx.x;
  if (tid == 0) sh.Psum = 0.f;
  if (tid < STDADK_MAX_Q) wS[tid] = 0.f;
  __syncthreads();
  for (int k = 1; k < Q; ++k) {
    float s = 0.f;
    for (int j = 1 + tid; j <= d; j += 256) s += fmaxf(-delta[k * ldd + j], 0.f);
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
      const float S = red[0] + red[1] + red[2] + red[3];
      const float d0 = delta[k * ldd];
      wS[k] = S > d0 ? 1.0f : (S == d0 ? 0.5f : 0.f);
      sh.Psum += d0 - fmaxf(d0, S);
    }
    __syncthreads();
  }
  float sq = 0.f;
  for (int j = tid; j <= d; j += 256) {
    float acc = 0.f;
    for (int k = Q - 1; k >= 0; --k) {
      acc += j == 0 ? dbo[k] : dWo[(int64_t)k * d + j - 1];
      float gp = 0.f;
      if (k >= 1) gp = j == 0 ? wS[k] : (delta[k * ldd + j] <= 0.f ? wS[k] : 0.f);
      const float g = fmaf(lam_g, gp, acc);
      d_delta[k * ldd + j] = g;
      if (SQ) sq = fmaf(g, g, sq);
    }
  }
  if (tid == 0 && loss_sum && lam_l != 0.f) atomicAdd(loss_sum, lam_l * sh.Psum);
  return sq;
}

}  // namespace stdadk
