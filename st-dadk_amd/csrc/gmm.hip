// One EM iteration of a spherical Gaussian mixture in two dimensions, entirely in float64 (stdadk_gmm_em_f64, see
// include/stdadk.h): the E-step on the parameters given, the M-step into a second parameter set.  The responsibilities
// r_ij = exp(lp_ij - lpn_i) are never stored: every pass recomputes lp_ij from the same expression (pair_lp, pinned with
// explicit fma so that the passes agree to the bit) and takes lpn_i from the workspace.  Four launches:
//   gmm_lpn_kernel     one thread per sample; the components pass through LDS in tiles of GMM_KT (centre and the two
//                      per-component constants of lp); running-maximum logsumexp in component order; lpn_i to the
//                      workspace, the workgroup's sum of lpn_i as one partial of the lower bound.
//   gmm_sums_kernel    workgroup (component j, sample slab s): sum_i r_ij, sum_i r_ij x_i over the slab, one thread per
//                      256th sample in sample order, then a fixed tree over the threads: one partial per (j, s).
//   gmm_var_kernel     the same grid: nk_j and mu_out_j from the slab partials added in slab order (every workgroup
//                      of a component forms the same bits; slab 0 writes mu_out), then sum_i r_ij |x_i - mu_out_j|^2
//                      over the slab -- non-negative terms about the NEW mean, a pass of its own.
//   gmm_finish_kernel  ONE workgroup: nk_j again, var_out_j, sum_j nk_j in a fixed order, w_out_j, the lower bound.
// No atomics, fixed orders (the tree is block_sum_f64 of f64_block.h): the same call on the same data gives the same
// bits.  Vector fp64 with exp / log; the work is n k pair evaluations per pass and at the sizes of the knot initialiser
// (10 000 x 121) it is bound by launch latency.
#include "f64_block.h"

namespace stdadk {

constexpr int GMM_T = 256;                 // threads per workgroup, every kernel
constexpr int GMM_KT = 256;                // components per LDS tile of gmm_lpn_kernel
constexpr int GMM_MAX_SLABS = 32;          // sample slabs per component, at most
constexpr int GMM_SLAB_FILL = 1024;        // slabs = ceil(GMM_SLAB_FILL / k): about this many workgroups when k is small
constexpr double GMM_LOG_2PI = 1.8378770664093453;
constexpr double GMM_NK_FLOOR = 10.0 * 2.220446049250313e-16;      // 10 eps, added to every nk_j
static_assert(GMM_T == 4 * kWave && GMM_KT == GMM_T, "gmm_lpn_kernel stages one component per thread");

// lp_ij = log w_j - 0.5 (2 log 2pi + |x_i - mu_j|^2 / var_j) - log var_j as  c_j - h_j |x_i - mu_j|^2  with
// c_j = log w_j - log 2pi - log var_j and h_j = 0.5 / var_j, the direct squared distance.
__device__ __forceinline__ double comp_c(double w, double var) { return (log(w) - GMM_LOG_2PI) - log(var); }
__device__ __forceinline__ double comp_h(double var) { return 0.5 / var; }
__device__ __forceinline__ double pair_lp(double x, double y, double mx, double my, double c, double h) {
  const double dx = x - mx, dy = y - my;
  const double lp = fma(-h, fma(dx, dx, dy * dy), c);
  return lp > -1e300 ? lp : -1e300;         // a weight of 0 (log = -inf) stays out of inf - inf
}

__global__ __launch_bounds__(GMM_T) void gmm_lpn_kernel(const double *__restrict__ X, int n, int k,
                                                        const double *__restrict__ w, const double *__restrict__ mu,
                                                        const double *__restrict__ var, double *__restrict__ lpn,
                                                        double *__restrict__ lb_part) {
  __shared__ double comp[GMM_KT][4];         // mx, my, c, h
  __shared__ double red[GMM_T];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * GMM_T + tid;
  const bool live = i < n;
  const double x = live ? X[2 * i] : 0.0, y = live ? X[2 * i + 1] : 0.0;
  double m = -__builtin_inf(), s = 0.0;
  for (int j0 = 0; j0 < k; j0 += GMM_KT) {
    const int nt = k - j0 < GMM_KT ? k - j0 : GMM_KT;
    __syncthreads();
    if (tid < nt) {
      const int j = j0 + tid;
      const double v = var[j];
      comp[tid][0] = mu[2 * j];
      comp[tid][1] = mu[2 * j + 1];
      comp[tid][2] = comp_c(w[j], v);
      comp[tid][3] = comp_h(v);
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const double lp = pair_lp(x, y, comp[t][0], comp[t][1], comp[t][2], comp[t][3]);
      if (lp > m) {
        s = fma(s, exp(m - lp), 1.0);        // the first component: 0 * exp(-inf) + 1
        m = lp;
      } else {
        s += exp(lp - m);
      }
    }
  }
  const double l = m + log(s);
  if (live) lpn[i] = l;
  const double tot = block_sum_f64<GMM_T>(red, live ? l : 0.0);
  if (tid == 0) lb_part[blockIdx.x] = tot;
}

struct GmmSlabs {
  int slabs, rows;                           // slab s holds the samples [s * rows, min(n, (s + 1) * rows))
};
static inline GmmSlabs gmm_slabs(int64_t n, int32_t k) {
  int64_t s = ceil_div(GMM_SLAB_FILL, k);
  const int64_t by_rows = ceil_div(n, GMM_T);
  if (s > by_rows) s = by_rows;
  if (s > GMM_MAX_SLABS) s = GMM_MAX_SLABS;
  if (s < 1) s = 1;
  GmmSlabs g;
  g.slabs = (int)s;
  g.rows = (int)ceil_div(n, s);
  return g;
}

__global__ __launch_bounds__(GMM_T) void gmm_sums_kernel(const double *__restrict__ X, int n, int rows,
                                                         const double *__restrict__ w, const double *__restrict__ mu,
                                                         const double *__restrict__ var,
                                                         const double *__restrict__ lpn, double *__restrict__ part) {
  __shared__ double red[GMM_T];
  const int j = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
  const double v = var[j], mx = mu[2 * j], my = mu[2 * j + 1];
  const double c = comp_c(w[j], v), h = comp_h(v);
  const int64_t i0 = (int64_t)sl * rows;
  const int64_t i1 = i0 + rows < n ? i0 + rows : n;
  double a0 = 0.0, ax = 0.0, ay = 0.0;
  for (int64_t i = i0 + tid; i < i1; i += GMM_T) {
    const double x = X[2 * i], y = X[2 * i + 1];
    const double r = exp(pair_lp(x, y, mx, my, c, h) - lpn[i]);
    a0 += r;
    ax = fma(r, x, ax);
    ay = fma(r, y, ay);
  }
  const double s0 = block_sum_f64<GMM_T>(red, a0), sx = block_sum_f64<GMM_T>(red, ax);
  const double sy = block_sum_f64<GMM_T>(red, ay);
  if (tid == 0) {
    double *p = part + ((size_t)j * gridDim.y + sl) * 3;
    p[0] = s0;
    p[1] = sx;
    p[2] = sy;
  }
}

// nk_j and the new mean from the slab partials, slabs added in slab order
__device__ __forceinline__ void comp_mean(const double *__restrict__ part, int j, int slabs, double &nk, double &mx,
                                          double &my) {
  double s0 = 0.0, sx = 0.0, sy = 0.0;
  for (int s = 0; s < slabs; ++s) {
    const double *p = part + ((size_t)j * slabs + s) * 3;
    s0 += p[0];
    sx += p[1];
    sy += p[2];
  }
  nk = s0 + GMM_NK_FLOOR;
  mx = sx / nk;
  my = sy / nk;
}

__global__ __launch_bounds__(GMM_T) void gmm_var_kernel(const double *__restrict__ X, int n, int rows,
                                                        const double *__restrict__ w, const double *__restrict__ mu,
                                                        const double *__restrict__ var,
                                                        const double *__restrict__ lpn,
                                                        const double *__restrict__ part, double *__restrict__ vpart,
                                                        double *__restrict__ mu_out) {
  __shared__ double red[GMM_T];
  const int j = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
  const double v = var[j], mx = mu[2 * j], my = mu[2 * j + 1];
  const double c = comp_c(w[j], v), h = comp_h(v);
  double nk, nx, ny;
  comp_mean(part, j, gridDim.y, nk, nx, ny);
  const int64_t i0 = (int64_t)sl * rows;
  const int64_t i1 = i0 + rows < n ? i0 + rows : n;
  double a = 0.0;
  for (int64_t i = i0 + tid; i < i1; i += GMM_T) {
    const double x = X[2 * i], y = X[2 * i + 1];
    const double r = exp(pair_lp(x, y, mx, my, c, h) - lpn[i]);
    const double ex = x - nx, ey = y - ny;
    a = fma(r, fma(ex, ex, ey * ey), a);
  }
  const double s = block_sum_f64<GMM_T>(red, a);
  if (tid == 0) {
    vpart[(size_t)j * gridDim.y + sl] = s;
    if (sl == 0) {
      mu_out[2 * j] = nx;
      mu_out[2 * j + 1] = ny;
    }
  }
}

__global__ __launch_bounds__(GMM_T) void gmm_finish_kernel(int n, int k, int slabs, int nblk, double reg_covar,
                                                           const double *__restrict__ part,
                                                           const double *__restrict__ vpart,
                                                           const double *__restrict__ lb_part,
                                                           double *__restrict__ w_out, double *__restrict__ var_out,
                                                           double *__restrict__ lower_bound) {
  __shared__ double red[GMM_T];
  const int tid = threadIdx.x;
  double tot = 0.0;
  for (int j = tid; j < k; j += GMM_T) {
    double nk, nx, ny;
    comp_mean(part, j, slabs, nk, nx, ny);
    double vs = 0.0;
    for (int s = 0; s < slabs; ++s) vs += vpart[(size_t)j * slabs + s];
    var_out[j] = vs / (2.0 * nk) + reg_covar;
    w_out[j] = nk;                             // divided by the total below, by the thread that wrote it
    tot += nk;
  }
  tot = block_sum_f64<GMM_T>(red, tot);
  for (int j = tid; j < k; j += GMM_T) w_out[j] = w_out[j] / tot;
  double lb = 0.0;
  for (int b = tid; b < nblk; b += GMM_T) lb += lb_part[b];
  lb = block_sum_f64<GMM_T>(red, lb);
  if (tid == 0) lower_bound[0] = lb / (double)n;
}

static inline bool gmm_sizes_ok(int64_t n, int32_t k) { return n >= 1 && n < (1ll << 31) && k >= 1 && k <= 65536; }

}  // namespace stdadk

using namespace stdadk;

// workspace: lpn [n], the lower bound's partials [ceil(n / GMM_T)], the slab partials [k][slabs][3] and [k][slabs]
extern "C" size_t stdadk_gmm_workspace_bytes(int64_t n, int32_t k) {
  if (!gmm_sizes_ok(n, k)) return 0;
  const GmmSlabs g = gmm_slabs(n, k);
  return ((size_t)n + (size_t)ceil_div(n, GMM_T) + (size_t)k * g.slabs * 4) * sizeof(double);
}

extern "C" int stdadk_gmm_em_f64(const double *X, int64_t n, int32_t k, const double *w, const double *mu,
                                 const double *var, double reg_covar, double *w_out, double *mu_out, double *var_out,
                                 double *lower_bound, void *workspace, size_t workspace_bytes, stdadk_stream_t stream) {
  STDADK_REQUIRE(n >= 1 && n < (1ll << 31), STDADK_E_ARG, "gmm_em: n=%lld outside 1..2^31-1", (long long)n);
  STDADK_REQUIRE(k >= 1 && k <= 65536, STDADK_E_ARG, "gmm_em: k=%d outside 1..65536", k);
  STDADK_REQUIRE(reg_covar > 0.0, STDADK_E_ARG, "gmm_em: reg_covar=%g must be positive", reg_covar);
  STDADK_REQUIRE(X && w && mu && var && w_out && mu_out && var_out && lower_bound && workspace, STDADK_E_ARG,
                 "gmm_em: NULL pointer");
  const size_t kb = (size_t)k * sizeof(double);
  const size_t need = stdadk_gmm_workspace_bytes(n, k);
  if (int rc = check_workspace("gmm_em", workspace, workspace_bytes, need, "stdadk_gmm_workspace_bytes")) return rc;
  const ByteRange in[] = {{X, (size_t)n * 2 * sizeof(double)}, {w, kb}, {mu, 2 * kb}, {var, kb}},
                  out[] = {{w_out, kb}, {mu_out, 2 * kb}, {var_out, kb}, {lower_bound, sizeof(double)}, {workspace, need}};
  if (int rc = check_no_alias("gmm_em", out, in, " (the caller ping-pongs two parameter sets)")) return rc;
  const GmmSlabs g = gmm_slabs(n, k);
  const int nblk = (int)ceil_div(n, GMM_T);
  double *lpn = (double *)workspace;
  double *lb_part = lpn + n;
  double *part = lb_part + nblk;
  double *vpart = part + (size_t)k * g.slabs * 3;
  hipStream_t st = (hipStream_t)stream;
  STDADK_LAUNCH(gmm_lpn_kernel, dim3((unsigned)nblk), dim3(GMM_T), 0, st, X, (int)n, (int)k, w, mu, var, lpn, lb_part);
  STDADK_CHECK_LAUNCH("gmm_lpn");
  STDADK_LAUNCH(gmm_sums_kernel, dim3((unsigned)k, (unsigned)g.slabs), dim3(GMM_T), 0, st, X, (int)n, g.rows, w, mu, var,
                (const double *)lpn, part);
  STDADK_CHECK_LAUNCH("gmm_sums");
  STDADK_LAUNCH(gmm_var_kernel, dim3((unsigned)k, (unsigned)g.slabs), dim3(GMM_T), 0, st, X, (int)n, g.rows, w, mu, var,
                (const double *)lpn, (const double *)part, vpart, mu_out);
  STDADK_CHECK_LAUNCH("gmm_var");
  STDADK_LAUNCH(gmm_finish_kernel, dim3(1), dim3(GMM_T), 0, st, (int)n, (int)k, g.slabs, nblk, reg_covar,
                (const double *)part, (const double *)vpart, (const double *)lb_part, w_out, var_out, lower_bound);
  STDADK_CHECK_LAUNCH("gmm_finish");
  return 0;
}
