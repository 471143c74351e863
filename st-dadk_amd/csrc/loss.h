// Batch objectives fused with their gradient (MSE, check loss + non-crossing penalty) and the
// delta-reparameterised head.  loss_elem() is the one arithmetic both the standalone kernel and
// the epilogue of the fused tail kernel use.
#pragma once
#include "common.h"

namespace stdadk {

struct LossDev {
  int kind;      // STDADK_LOSS_*
  int y_cols;    // 1 or Q
  float tau[STDADK_MAX_Q];
  float nc_w;    // 0 = off
  int nc_pow;    // 1 or 2
};

// NULL = MSE against y [B,Q].  Returns non-zero (error text set) on a bad descriptor.
int make_loss(const stdadk_loss_desc *l, int Q, LossDev *out);
inline bool loss_is_plain_mse(const LossDev &L, int Q) { return L.kind == STDADK_LOSS_MSE && L.y_cols == Q; }

int launch_loss(const LossDev &L, const float *yp, const float *y, int64_t B, int Q, float scale, float *dY,
                float *loss_sum, hipStream_t st);

// the derived output layer of the delta head (stdadk_delta_head_f32): Wo [Q,d], bo [Q] from delta [Q, ldd]
int launch_delta_head(const float *delta, int64_t ldd, int Q, int d, float *Wo, float *bo, hipStream_t st);

// tau of output q without indexing the kernel-argument array by a vector register
__device__ __forceinline__ float loss_tau(const LossDev &L, int q) {
  float t = L.tau[0];
#pragma unroll
  for (int k = 1; k < STDADK_MAX_Q; ++k) t = q == k ? L.tau[k] : t;
  return t;
}

// One (row, q) element: prediction yq, its neighbours yup = y_pred[q+1], ydn = y_pred[q-1] (read only
// when they exist), target yt.  Returns the element's share of the loss sum, dy = its gradient.
__device__ __forceinline__ float loss_elem(const LossDev &L, int Q, int q, float tau, float yq, float yup,
                                           float ydn, float yt, float gs, float &dy) {
  if (L.kind == STDADK_LOSS_MSE) {
    const float d = yq - yt;
    dy = 2.0f * d * gs;
    return d * d;
  }
  const float e = yt - yq;
  float term = fmaxf((tau - 1.0f) * e, tau * e);
  float g = e > 0.f ? -tau : (e < 0.f ? 1.0f - tau : 0.5f - tau);
  if (L.nc_w > 0.f) {
    float f = 0.f, gn = 0.f;
    if (q + 1 < Q) {
      const float d = yq - yup;
      if (d > 0.f) { f = L.nc_pow == 1 ? d : d * d; gn = L.nc_pow == 1 ? 1.0f : 2.0f * d; }
    }
    if (q > 0) {
      const float d = ydn - yq;
      if (d > 0.f) gn -= L.nc_pow == 1 ? 1.0f : 2.0f * d;
    }
    const float w = L.nc_w * (float)Q;
    term = fmaf(w, f, term);
    g = fmaf(w, gn, g);
  }
  dy = g * gs;
  return term;
}

// One (row, q) element of the check loss on its own (validation metrics): max((tau-1) e, tau e), e = y - y_pred.
__device__ __forceinline__ float check_elem(float tau, float yq, float yt) {
  const float e = yt - yq;
  return fmaxf((tau - 1.0f) * e, tau * e);
}
// the same term in double (grid scores, grid_score.hip)
__device__ __forceinline__ double check_elem(double tau, double yq, double yt) {
  const double e = yt - yq;
  return fmax((tau - 1.0) * e, tau * e);
}

// Validation metrics of one batch (eval.hip): values a workgroup leaves per partial -- objective, squared and absolute
// error of the metric column, per-level check loss.
constexpr int EVAL_V_OBJ = 0, EVAL_V_SSE = 1, EVAL_V_SAE = 2, EVAL_V_CHECK = 3;
constexpr int EVAL_VALS = EVAL_V_CHECK + STDADK_MAX_Q;
constexpr int EVAL_MAX_WG = 1024;
int eval_partials_blocks(int64_t B);
// yp [B,Q] and y [B, L.y_cols] in the SAME row order (any); part: EVAL_MAX_WG * EVAL_VALS doubles of scratch;
// acc: the STDADK_EVAL_SLOTS doubles stdadk_eval_indexed_f32 adds into.
int launch_eval_metrics(const LossDev &L, const float *yp, const float *y, int64_t B, int Q, int metric_col,
                        double batch_weight, double *part, double *acc, hipStream_t st);

}  // namespace stdadk
