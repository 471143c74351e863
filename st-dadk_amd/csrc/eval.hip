// Validation metrics (stdadk_eval_indexed_f32, see include/stdadk.h): the deterministic reduction of one batch's
// predictions against its targets into the float64 accumulator.  Two launches:
//   eval_partials_kernel  one thread per row (its Q predictions are consecutive: a wave reads one contiguous span),
//                         float sums per thread, DPP wave sums, one double partial per value and workgroup;
//   eval_finish_kernel    ONE workgroup: the partials of every value added in double in a fixed order, then added
//                         into the accumulator by one thread (stream order makes the read-modify-write safe).
// No atomics anywhere: the same call on the same data gives the same bits.  Fusing this into the tail kernel's
// epilogue was not pursued: the predictions are B*Q*4 bytes beside a forward that moves B*(sum of widths)*4, and the
// tail's instantiations are shared with training ("Validation").
#include "loss.h"

namespace stdadk {

constexpr int EVAL_T = 256;
static_assert(EVAL_T == 4 * kWave, "eval_partials_kernel adds the partials of exactly four waves");

__global__ __launch_bounds__(EVAL_T) void eval_partials_kernel(LossDev L, const float *__restrict__ yp,
                                                              const float *__restrict__ y, int B, int Q, int mcol,
                                                              double *__restrict__ part) {
  float acc[EVAL_VALS];
#pragma unroll
  for (int k = 0; k < EVAL_VALS; ++k) acc[k] = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * EVAL_T + threadIdx.x; row < B; row += (int64_t)gridDim.x * EVAL_T) {
    float p[STDADK_MAX_Q], yt[STDADK_MAX_Q];
    const float y0 = L.y_cols == 1 ? y[row] : 0.f;
#pragma unroll
    for (int q = 0; q < STDADK_MAX_Q; ++q) {
      p[q] = q < Q ? yp[row * Q + q] : 0.f;
      yt[q] = L.y_cols == 1 ? y0 : (q < Q ? y[row * Q + q] : 0.f);
    }
    float pm = p[0], ym = yt[0];
#pragma unroll
    for (int q = 1; q < STDADK_MAX_Q; ++q) { pm = q == mcol ? p[q] : pm; ym = q == mcol ? yt[q] : ym; }
    const float dm = pm - ym;
    acc[EVAL_V_SSE] = fmaf(dm, dm, acc[EVAL_V_SSE]);
    acc[EVAL_V_SAE] += fabsf(dm);
#pragma unroll
    for (int q = 0; q < STDADK_MAX_Q; ++q) {
      if (q < Q) {
        float dy;
        acc[EVAL_V_OBJ] += loss_elem(L, Q, q, L.tau[q], p[q], q + 1 < STDADK_MAX_Q ? p[q + 1] : 0.f,
                                     q > 0 ? p[q - 1] : 0.f, yt[q], 0.f, dy);
        acc[EVAL_V_CHECK + q] += check_elem(L.tau[q], p[q], yt[q]);
      }
    }
  }
  __shared__ float red[EVAL_T / kWave][EVAL_VALS];
#pragma unroll
  for (int k = 0; k < EVAL_VALS; ++k) {
    const float s = wave_sum(acc[k]);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < EVAL_VALS) {
    const int k = threadIdx.x;
    part[(size_t)blockIdx.x * EVAL_VALS + k] = ((double)red[0][k] + (double)red[1][k]) + ((double)red[2][k] + (double)red[3][k]);
  }
}

__global__ __launch_bounds__(EVAL_T) void eval_finish_kernel(const double *__restrict__ part, int nblk, int Q,
                                                            double weight, double rows, double *__restrict__ acc) {
  __shared__ double red[EVAL_T];
  const int tid = threadIdx.x;
  for (int k = 0; k < EVAL_VALS; ++k) {
    if (k >= EVAL_V_CHECK + Q) break;
    double s = 0.0;
    for (int i = tid; i < nblk; i += EVAL_T) s += part[(size_t)i * EVAL_VALS + k];
    red[tid] = s;
    __syncthreads();
    for (int o = EVAL_T / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) {
      const int slot = k == EVAL_V_OBJ ? STDADK_EVAL_OBJECTIVE
                                       : (k == EVAL_V_SSE ? STDADK_EVAL_SSE
                                                          : (k == EVAL_V_SAE ? STDADK_EVAL_SAE
                                                                             : STDADK_EVAL_CHECK + (k - EVAL_V_CHECK)));
      acc[slot] += k == EVAL_V_OBJ ? weight * red[0] : red[0];
    }
    __syncthreads();
  }
  if (tid == 0) {
    acc[STDADK_EVAL_ROWS] += rows;
    acc[STDADK_EVAL_BATCHES] += 1.0;
  }
}

int eval_partials_blocks(int64_t B) {
  int64_t n = ceil_div(B > 0 ? B : 1, EVAL_T);
  return (int)(n > EVAL_MAX_WG ? EVAL_MAX_WG : n);
}

int launch_eval_metrics(const LossDev &L, const float *yp, const float *y, int64_t B, int Q, int metric_col,
                        double batch_weight, double *part, double *acc, hipStream_t st) {
  const int nblk = eval_partials_blocks(B);
  STDADK_LAUNCH(eval_partials_kernel, dim3((unsigned)nblk), dim3(EVAL_T), 0, st, L, yp, y, (int)B, Q, metric_col, part);
  STDADK_CHECK_LAUNCH("eval_partials");
  STDADK_LAUNCH(eval_finish_kernel, dim3(1), dim3(EVAL_T), 0, st, (const double *)part, nblk, Q, batch_weight,
                (double)B, acc);
  STDADK_CHECK_LAUNCH("eval_finish");
  return 0;
}

}  // namespace stdadk
