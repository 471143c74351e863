// The finishing launch of a one-call learnable-knot step (stdadk_train_step_knots_f32): what closes the gradients of
// BOTH parameter groups and leaves both clip norms -- the step's fixed-order sums (reduce_jobs_kernel's workgroups)
// and the knot finish (knot_finish_kernel's tiles) as one kernel.
#pragma once
#include "gemm_f32.h"
#include "knots.h"

namespace stdadk {

// knot workgroups of the launch: one per 64-knot tile, at most STDADK_SUMSQ_PARTS (they stride over the tiles)
int step_finish_knot_blocks(int Ks);

// Workgroups [0, reduce_jobs_block_count(grp)) run the reduce jobs of `grp` (possibly none) and leave grp.sq_parts
// when it is set, exactly as launch_reduce_jobs does (grp.sq_region_parts / grp.step_inc must be NULL); the
// step_finish_knot_blocks(a.Ks) workgroups behind them finish the knots.  knot_parts (or NULL): all
// STDADK_SUMSQ_PARTS entries are written -- [w] = squares of the d_centers / d_log_bw entries knot workgroup w wrote,
// zeros behind the last workgroup.  step_inc (or NULL) is advanced by one.
int launch_step_finish(ReduceGroup &grp, const KnotFinishArgs &a, float *knot_parts, int *step_inc, hipStream_t st);

}  // namespace stdadk
