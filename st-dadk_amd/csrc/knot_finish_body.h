// The knot finish of one tile of 64 knots (see knots.h: KnotFinishArgs), shared by knot_finish_kernel (knots.hip:
// one tile per workgroup) and step_finish_kernel (step_finish.hip: the knot workgroups of the finishing launch of a
// one-call learnable step stride over the tiles).
#pragma once
#include "knots.h"

namespace stdadk {

// per knot: fixed-order sum of the slab partials, + penalty gradients, x damping factor; the tile's penalty value goes
// into a.loss_sum.  256 threads: the 4 waves each sum every 4th slab (independent loads), the four partial sums meet
// in `part`; `red`: 4 floats.  Returns (wave 0, knots below Ks; 0 elsewhere) the squares of the three gradient entries
// the thread wrote.  A caller that runs it again on another tile puts a barrier in between (`part` and `red`).
__device__ __forceinline__ float knot_finish_tile(const KnotFinishArgs &a, const int tile, float (*part)[4][64],
                                                  float *red) {
  const int kl = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int k = tile * 64 + kl;
  float gx = 0.f, gy = 0.f, gl = 0.f;
  if (k < a.Ks) {
    for (int s = sg; s < a.slabs; s += 4) {
      gx += a.part[((size_t)s * 3 + 0) * a.Ks + k];
      gy += a.part[((size_t)s * 3 + 1) * a.Ks + k];
      gl += a.part[((size_t)s * 3 + 2) * a.Ks + k];
    }
  }
  part[0][sg][kl] = gx; part[1][sg][kl] = gy; part[2][sg][kl] = gl;
  __syncthreads();
  float pen = 0.f, sq = 0.f;
  if (sg == 0 && k < a.Ks) {
    gx = (part[0][0][kl] + part[0][1][kl]) + (part[0][2][kl] + part[0][3][kl]);
    gy = (part[1][0][kl] + part[1][1][kl]) + (part[1][2][kl] + part[1][3][kl]);
    gl = (part[2][0][kl] + part[2][1][kl]) + (part[2][2][kl] + part[2][3][kl]);
    const float cx = a.centers[2 * k], cy = a.centers[2 * k + 1];
    float mx = 0.f, my = 0.f;
    if (a.centers_init) { mx = cx - a.centers_init[2 * k]; my = cy - a.centers_init[2 * k + 1]; }
    if (a.dom_w > 0.f) {
      // (max(0, 0-c) + max(0, c-1))^2 per coordinate (st_interp.py:511-524)
      const float vx = fmaxf(0.f - cx, 0.f) + fmaxf(cx - 1.0f, 0.f);
      const float vy = fmaxf(0.f - cy, 0.f) + fmaxf(cy - 1.0f, 0.f);
      pen = fmaf(a.dom_w, vx * vx + vy * vy, pen);
      gx = fmaf(a.pen_grad_scale * a.dom_w, 2.0f * vx * (cx > 1.0f ? 1.0f : (cx < 0.f ? -1.0f : 0.f)), gx);
      gy = fmaf(a.pen_grad_scale * a.dom_w, 2.0f * vy * (cy > 1.0f ? 1.0f : (cy < 0.f ? -1.0f : 0.f)), gy);
    }
    if (a.mov_w > 0.f) {
      pen = fmaf(a.mov_w, mx * mx + my * my, pen);
      gx = fmaf(a.pen_grad_scale * a.mov_w, 2.0f * mx, gx);
      gy = fmaf(a.pen_grad_scale * a.mov_w, 2.0f * my, gy);
    }
    if (a.damping) {
      const float dist = __builtin_amdgcn_sqrtf(fmaf(mx, mx, my * my));
      const float f = expf(-a.strength * fmaxf(dist - a.thr, 0.f));
      gx *= f; gy *= f;
    }
    a.d_centers[2 * k] = gx; a.d_centers[2 * k + 1] = gy;
    a.d_log_bw[k] = gl;
    sq = (gx * gx + gy * gy) + gl * gl;
  }
  if (a.loss_sum && a.pen_loss_scale != 0.f && (a.dom_w > 0.f || a.mov_w > 0.f)) {
    const float s = wave_sum(pen);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(a.loss_sum, a.pen_loss_scale * ((red[0] + red[1]) + (red[2] + red[3])));
  }
  return sq;
}

}  // namespace stdadk
