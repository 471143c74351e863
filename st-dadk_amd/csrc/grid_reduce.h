// What the reductions over a site x time grid share (grid_score.hip, quantile_diag.hip): one thread owns a site, so a
// workgroup is GS_T sites; a value is summed over a wave's lanes by a fixed DPP tree in double, and the partial rows a
// first launch leaves per workgroup are added in a fixed order by a second one.  No atomics anywhere.
#pragma once
#include "common.h"

namespace stdadk {

constexpr int GS_T = 256;                   // sites per workgroup
constexpr int GS_W = GS_T / kWave;          // waves per workgroup

// wave_sum (common.h) on a double: the same DPP tree on both halves of the value
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_f64(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t l = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, ROW_MASK, 0xF, false);
  const uint32_t h = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, ROW_MASK, 0xF, false);
  return __builtin_bit_cast(double, ((uint64_t)h << 32) | l);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  v += dpp_f64<0x142, 0xA>(v);
  v += dpp_f64<0x143, 0xC>(v);
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, 63);
  const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), 63);
  return __builtin_bit_cast(double, ((uint64_t)h << 32) | l);
}

// NV values per partial row, G = GS_T / NV groups of threads stride over the rows, then one thread per value adds the
// groups' sums in order.  row(i) = the i-th partial row of this reduction.
template <int NV, typename RowFn>
__device__ __forceinline__ double sum_partials(double *red, int nrows, RowFn row) {
  constexpr int G = GS_T / NV;
  const int tid = threadIdx.x, k = tid % NV, g = tid / NV;
  if (g < G) {
    double s = 0.0;
    for (int i = g; i < nrows; i += G) s += row(i)[k];
    red[g * NV + k] = s;
  }
  __syncthreads();
  double s = 0.0;
  if (tid < NV)
    for (int j = 0; j < G; ++j) s += red[j * NV + tid];
  return s;
}

static inline int64_t grid_score_blocks(int64_t S) { return ceil_div(S > 0 ? S : 1, GS_T); }

// ---- host side: what stdadk_grid_score_f32 and stdadk_quantile_diag_f32 ask of their arguments ----

// S, nT and the row count S nT fit 31 bits (the kernels index rows with int)
static inline bool grid_sizes_ok(int64_t S, int64_t nT) {
  return S >= 0 && nT >= 0 && S < (1ll << 31) && nT < (1ll << 31) && S * nT < (1ll << 31);
}

// The checks after the NULL test, in this order: Q, the metric column (0 from a caller that has none), the interval
// columns, the sizes, the workspace (`need` bytes, as `sizer` computes them).
static inline int check_grid_args(const char *who, int64_t S, int64_t nT, int32_t Q, int32_t metric_col, int32_t lo_col,
                                  int32_t hi_col, const void *workspace, size_t have, size_t need, const char *sizer) {
  STDADK_REQUIRE(Q >= 1 && Q <= STDADK_MAX_Q, STDADK_E_ARG, "%s: Q=%d outside 1..%d", who, Q, STDADK_MAX_Q);
  STDADK_REQUIRE(metric_col >= 0 && metric_col < Q, STDADK_E_ARG, "%s: metric_col=%d outside 0..%d", who, metric_col, Q - 1);
  STDADK_REQUIRE((lo_col == -1 && hi_col == -1) || (lo_col >= 0 && hi_col < Q && lo_col < hi_col), STDADK_E_ARG,
                 "%s: interval columns (%d, %d) must be (-1, -1) or 0 <= lo < hi < Q=%d", who, lo_col, hi_col, Q);
  STDADK_REQUIRE(grid_sizes_ok(S, nT), STDADK_E_SHAPE, "%s: S*nT = %lld x %lld rows do not fit 31 bits", who, (long long)S,
                 (long long)nT);
  return check_workspace(who, workspace, have, need, sizer);
}

// the kernels' levels: the caller's Q, 0.5 each without any, 0.5 past Q
static inline void fill_taus(float (&tau)[STDADK_MAX_Q], const float *taus_host, int Q) {
  for (int q = 0; q < STDADK_MAX_Q; ++q) tau[q] = taus_host && q < Q ? taus_host[q] : 0.5f;
}

// STDADK_LAUNCH of the instantiation kern<Q> for Q in 1..STDADK_MAX_Q (checked before); the rest are its arguments
#define STDADK_GRID_Q_CASE(kern, q, ...)   \
  case q:                                  \
    STDADK_LAUNCH(kern<q>, __VA_ARGS__);   \
    break;
#define STDADK_LAUNCH_FOR_Q(Q, kern, ...)                                                         \
  switch (Q) {                                                                                    \
    STDADK_GRID_Q_CASE(kern, 1, __VA_ARGS__) STDADK_GRID_Q_CASE(kern, 2, __VA_ARGS__)            \
    STDADK_GRID_Q_CASE(kern, 3, __VA_ARGS__) STDADK_GRID_Q_CASE(kern, 4, __VA_ARGS__)            \
    STDADK_GRID_Q_CASE(kern, 5, __VA_ARGS__) STDADK_GRID_Q_CASE(kern, 6, __VA_ARGS__)            \
    STDADK_GRID_Q_CASE(kern, 7, __VA_ARGS__) STDADK_GRID_Q_CASE(kern, 8, __VA_ARGS__)            \
  }
static_assert(STDADK_MAX_Q == 8, "STDADK_LAUNCH_FOR_Q lists the instantiations");

}  // namespace stdadk
