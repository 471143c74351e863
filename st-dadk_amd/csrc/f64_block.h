// What the float64 knot initialisers share on the device (gmm.hip, kmeans.hip, kmeanspp.hip): the squared distance of
// k-means and the fixed trees over a workgroup of T threads.  Their contract is the same bits on every call -- fixed
// orders, no atomics -- and the bits of the distance are also what the host restatements of the tests form.
#pragma once
#include "common.h"

namespace stdadk {

// |(x, y) - (cx, cy)|^2 with every operation rounded once: two differences, two products, one sum.  Contraction is off
// because a fused multiply-add would round dx dx + dy dy once instead of twice, and then neither a float64 restatement
// on the host (numpy never fuses) nor another kernel that reaches the same pair would form the same bits: the
// quantised costs of kmeans.hip and the picks of kmeanspp.hip are decided by the last bit of this value.
__device__ __forceinline__ double sq_dist_f64(double x, double y, double cx, double cy) {
#pragma clang fp contract(off)
  const double dx = x - cx, dy = y - cy;
  const double a = dx * dx, b = dy * dy;
  return a + b;
}

// Sum over the T threads of a workgroup by a fixed tree through red[T]; the sum comes back in every thread.  The
// leading barrier lets a kernel call it again on the same array.
template <int T>
__device__ __forceinline__ double block_sum_f64(double *red, double v) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = T / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// Maximum over the T threads by the same tree; it comes back in every thread.  NO leading barrier: every kernel that
// calls it uses its red array for this one reduction only.
template <int T>
__device__ __forceinline__ double block_max_f64(double *red, double v) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = T / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] > red[tid + o] ? red[tid] : red[tid + o];
    __syncthreads();
  }
  return red[0];
}

}  // namespace stdadk
