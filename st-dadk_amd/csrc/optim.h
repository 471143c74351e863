// internal: the one host path behind every AdamW launch (optim.hip): one or two parameter groups (stdadk_adam_group:
// what differs per group) under one set of hyper-parameters (AdamHyper: what the groups share)
#pragma once
#include "common.h"

namespace stdadk {
struct BinSmallArgs;

struct AdamHyper {
  float beta1, beta2, eps, weight_decay;
  int32_t step; const int32_t *step_dev;             // the step being applied: step_dev[0] when given, else `step`
  float grad_mul, ema_decay;
  const float *loss_watch; int32_t *nonfinite_step;  // non-finite guard (stdadk.h): both or neither
};

// the group and hyper-parameters of a one-call step, whose launches have advanced o->step_dev: clip partials `parts`
// (NULL = no clipping), the guard of `o` watching `loss_sum`
static inline void optim_group(const stdadk_optim_desc *o, const float *parts, int32_t n_parts, const float *loss_sum,
                               stdadk_adam_group *gr, AdamHyper *h) {
  *gr = {o->p, o->g, o->m, o->v, o->ema, o->n, o->lr, o->lr_dev, o->max_norm, parts, n_parts, o->shadow};
  *h = {o->beta1, o->beta2, o->eps, o->weight_decay, 1, o->step_dev, 1.0f, o->ema_decay,
        o->nonfinite_step ? loss_sum : nullptr, o->nonfinite_step};
}

// Validates `ng` (1 or 2) groups -- errors are reported under the prefix `what` -- and steps them in ONE launch:
// adamw_ema_kernel, adamw_ema2_kernel or, with `bin` (one group only), adamw_bin_kernel, whose extra workgroups bin
// the next batch.  A single group may be empty (nothing is launched); the first group's workgroups keep the guard.
// `pack_f32` (STDADK_FLAG_PACK_F32 of a one-call step): the groups' shadow tables name fragment-order fp32 copies.
int adamw_launch(const char *what, int ng, const stdadk_adam_group *g0, const stdadk_adam_group *g1, const AdamHyper &h,
                 const BinSmallArgs *bin, stdadk_stream_t stream, bool pack_f32 = false);
}  // namespace stdadk
