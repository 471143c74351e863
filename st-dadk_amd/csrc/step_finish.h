// The finishing launch of a one-call step with more than the plain MLP group to close (stdadk_train_step_knots_f32,
// stdadk_train_step_delta_f32): what closes the gradients of every parameter group and leaves their clip norms -- the
// step's fixed-order sums (reduce_jobs_kernel's workgroups), the knot finish (knot_finish_kernel's tiles) and the
// backward of the delta head (delta_head_bwd_kernel's workgroup) as one kernel of three kinds of workgroup.
#pragma once
#include "gemm_f32.h"
#include "knots.h"

namespace stdadk {

// The head workgroup (delta step): folds the output layer's gradient (dWo, dbo) into the delta rows of the flat gradient
// with the gradient and value of P_nc(delta), as stdadk_delta_head_backward_f32 does.  `pending`: dWo / dbo are still
// the column partials of the row-local launch and no launch in front of this one sums them -- the workgroup first runs
// their two reduce jobs itself, eight blocks of 16 columns at a time, in reduce_job_block's per-element order (no
// hand-over between workgroups inside the launch); 0: they are final (generic kernels; or a reductions launch / the
// weight-gradient launch in finishing mode 2 ran in front: zero_slots).
struct HeadFinishArgs {
  float *d_delta = nullptr;       // [Q, ldd]; NULL: the launch has no head workgroup
  const float *delta = nullptr;   // [Q, ldd]
  const float *dWo = nullptr, *dbo = nullptr;
  int64_t ldd = 0;
  int Q = 0, d = 0;
  float lam_g = 0.f, lam_l = 0.f;
  float *loss_sum = nullptr;
  float *sq_part = nullptr;       // ONE partial: the squares of the d_delta entries written (NULL: not wanted)
  int pending = 0;
  float *zero_slots = nullptr;    // pending == 0 behind the fused tail kernels: a launch in front ran the output layer's
  int n_zero = 0;                 // two sums WITH the others and left their squares in these slots -- cleared here
  ReduceJob job[2];               // dst = dWo / dbo
  int nblk[2] = {0, 0};           // set by launch_step_finish
};

// knot workgroups of the launch: one per 64-knot tile, at most STDADK_SUMSQ_PARTS (they stride over the tiles)
int step_finish_knot_blocks(int Ks);

// Workgroups [0, reduce_jobs_block_count(grp)) run the reduce jobs of `grp` (possibly none) and leave grp.sq_parts
// when it is set, exactly as launch_reduce_jobs does (grp.sq_region_parts / grp.step_inc must be NULL); the
// step_finish_knot_blocks(a.Ks) workgroups behind them finish the knots (a.Ks == 0: fixed knots, none); the last
// workgroup is the head's when h.d_delta is set.  knot_parts (or NULL): all STDADK_SUMSQ_PARTS entries are written --
// [w] = squares of the d_centers / d_log_bw entries knot workgroup w wrote, zeros behind the last workgroup.
// step_inc (or NULL) is advanced by one.
int launch_step_finish(ReduceGroup &grp, const KnotFinishArgs &a, float *knot_parts, int *step_inc, hipStream_t st,
                       const HeadFinishArgs *h = nullptr);

}  // namespace stdadk
