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

}  // namespace stdadk
