// Scores of a site x time prediction grid (stdadk_grid_score_f32, see include/stdadk.h): one chunk of nT time slices of
// predictions [nT*S][Q] reduced against the field z [nT][S] and the split codes into float64 sums per split, per
// (split, site) and per (split, time).  Three launches:
//   grid_score_kernel        one thread owns a SITE (lanes run along s: y_pred, z and split are read in contiguous
//                            spans) and walks the chunk's slices in time order.  Its 4 x 3 site sums live in registers,
//                            START from site_acc and go back there, so a site's slices are added one by one in time order
//                            however the grid is cut into chunks (stream order between the calls makes the
//                            read-modify-write safe).  Per slice the wave's (sse, sae, n) of every split are summed over
//                            the lanes (DPP, fixed tree), the four waves' values are added through LDS in tiles of
//                            GS_TT slices and leave as one partial per (workgroup, slice).  The per-split check-loss,
//                            cover and width sums stay in registers for the whole chunk and leave as one partial per
//                            workgroup.
//   grid_score_time_kernel   workgroup ti < nT: the partials of slice ti over the workgroups, fixed order, ASSIGNED to
//                            time_acc; workgroup nT: the check / cover / width partials, added into split_acc.
//   grid_score_split_kernel  n, sse, sae of every split = the chunk's time_acc summed over its slices, added into split_acc.
// Every element term is formed in double from operands converted to double; no atomics anywhere: the same call on the
// same data gives the same bits.  The kernel reads 4Q + 5 bytes per grid entry and is bound by that.
#include "grid_reduce.h"
#include "loss.h"

namespace stdadk {

constexpr int GS_TT = 16;                   // slices per LDS tile
constexpr int GS_TV = 12;                   // values per slice: 4 splits x (sse, sae, n)
constexpr int GS_X = STDADK_MAX_Q + 2;      // chunk-long values per split: check[q], cover, width
constexpr int GS_XV = 4 * GS_X;
static_assert(GS_W == 4 && GS_TT % 8 == 0 && GS_TT * GS_TV <= GS_T && GS_XV <= GS_T, "grid_score_kernel's LDS hand-over");
static_assert(STDADK_GRID_CHECK + STDADK_MAX_Q <= STDADK_GRID_SLOTS, "per-split slots");

struct GridScoreArgs {
  const float *yp, *z;
  const uint8_t *split;
  int S, nT, mcol, lo, hi;
  float tau[STDADK_MAX_Q];
  double *site_acc, *tpart, *xpart;
};

template <int Q>
__global__ __launch_bounds__(GS_T) void grid_score_kernel(GridScoreArgs a) {
  __shared__ double red[GS_TT][GS_W][GS_TV];
  static_assert(GS_TT * GS_TV >= GS_XV, "the chunk-long values reuse the tile");
  constexpr int GS_U = Q <= 4 ? 8 : 4;  // slices whose loads are issued together (registers: GS_U * (Q + 2))
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int s = blockIdx.x * GS_T + tid;
  const bool live = s < a.S;            // the threads past the last site stay in every wave sum, adding nothing
  const bool interval = a.lo >= 0;
  double sa[4][3], xa[4][Q + 2];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int v = 0; v < 3; ++v) sa[c][v] = live ? a.site_acc[((size_t)c * a.S + s) * 3 + v] : 0.0;
#pragma unroll
    for (int j = 0; j < Q + 2; ++j) xa[c][j] = 0.0;
  }
  for (int t0 = 0; t0 < a.nT; t0 += GS_TT) {
    const int nt = a.nT - t0 < GS_TT ? a.nT - t0 : GS_TT;
#pragma unroll
    for (int u0 = 0; u0 < GS_TT; u0 += GS_U) {
      if (u0 >= nt) break;
      float zf[GS_U], p[GS_U][Q];
      int code[GS_U];
#pragma unroll
      for (int u = 0; u < GS_U; ++u) {
        const bool on = live && u0 + u < nt;
        const size_t row = (size_t)(t0 + u0 + u) * a.S + s;
        zf[u] = on ? a.z[row] : __builtin_nanf("");
        code[u] = on && a.split ? (int)a.split[row] : 0;
#pragma unroll
        for (int q = 0; q < Q; ++q) p[u][q] = on ? a.yp[row * Q + q] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < GS_U; ++u) {
        if (u0 + u >= nt) break;
        const bool ok = zf[u] - zf[u] == 0.f;            // finite: NaN and +-inf count nowhere
        const double zd = (double)zf[u];
        float pm = p[u][0], pl = p[u][0], ph = p[u][0];
#pragma unroll
        for (int q = 1; q < Q; ++q) {
          pm = q == a.mcol ? p[u][q] : pm;
          pl = q == a.lo ? p[u][q] : pl;
          ph = q == a.hi ? p[u][q] : ph;
        }
        const double d = (double)pm - zd;
        const double e2 = d * d, e1 = fabs(d);
        const double wd = (double)ph - (double)pl;
        const double cov = ((double)pl <= zd && zd <= (double)ph) ? 1.0 : 0.0;
        double ck[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) ck[q] = check_elem((double)a.tau[q], (double)p[u][q], zd);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool m = ok && code[u] == c;
          const double m2 = m ? e2 : 0.0, m1 = m ? e1 : 0.0;
          sa[c][0] += m2;
          sa[c][1] += m1;
          sa[c][2] += m ? 1.0 : 0.0;
#pragma unroll
          for (int q = 0; q < Q; ++q) xa[c][q] += m ? ck[q] : 0.0;
          xa[c][Q] += m && interval ? cov : 0.0;
          xa[c][Q + 1] += m && interval ? wd : 0.0;
          const double w2 = wave_sum_f64(m2), w1 = wave_sum_f64(m1);
          const double wn = (double)__builtin_popcountll(__ballot(m));
          if (lane == 0) {
            red[u0 + u][wave][c * 3 + 0] = w2;
            red[u0 + u][wave][c * 3 + 1] = w1;
            red[u0 + u][wave][c * 3 + 2] = wn;
          }
        }
      }
    }
    __syncthreads();
    if (tid < nt * GS_TV) {
      const int tl = tid / GS_TV, k = tid % GS_TV;
      a.tpart[((size_t)blockIdx.x * a.nT + t0 + tl) * GS_TV + k] =
          (red[tl][0][k] + red[tl][1][k]) + (red[tl][2][k] + red[tl][3][k]);
    }
    __syncthreads();
  }
  if (live) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int v = 0; v < 3; ++v) a.site_acc[((size_t)c * a.S + s) * 3 + v] = sa[c][v];
  }
  double *xr = &red[0][0][0];           // [GS_W][GS_XV]
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int j = 0; j < GS_X; ++j) {
      // slots of a split: check[0..MAX_Q), cover, width
      const int r = j < Q ? j : (j == STDADK_MAX_Q ? Q : (j == STDADK_MAX_Q + 1 ? Q + 1 : -1));
      const double w = r >= 0 ? wave_sum_f64(xa[c][r >= 0 ? r : 0]) : 0.0;
      if (lane == 0) xr[wave * GS_XV + c * GS_X + j] = w;
    }
  }
  __syncthreads();
  if (tid < GS_XV)
    a.xpart[(size_t)blockIdx.x * GS_XV + tid] =
        (xr[tid] + xr[GS_XV + tid]) + (xr[2 * GS_XV + tid] + xr[3 * GS_XV + tid]);
}

__global__ __launch_bounds__(GS_T) void grid_score_time_kernel(const double *__restrict__ tpart,
                                                              const double *__restrict__ xpart, int nblk, int nT, int Q,
                                                              int interval, double *__restrict__ time_acc,
                                                              double *__restrict__ split_acc) {
  __shared__ double red[GS_T];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < nT) {
    const int ti = blockIdx.x;
    const double s = sum_partials<GS_TV>(red, nblk, [&](int i) { return tpart + ((size_t)i * nT + ti) * GS_TV; });
    if (tid < GS_TV) time_acc[((size_t)(tid / 3) * nT + ti) * 3 + tid % 3] = s;
    return;
  }
  const double s = sum_partials<GS_XV>(red, nblk, [&](int i) { return xpart + (size_t)i * GS_XV; });
  if (tid < GS_XV) {
    const int c = tid / GS_X, j = tid % GS_X;
    double *acc = split_acc + (size_t)c * STDADK_GRID_SLOTS;
    if (j < Q) acc[STDADK_GRID_CHECK + j] += s;
    if (j == STDADK_MAX_Q && interval) acc[STDADK_GRID_COVER] += s;
    if (j == STDADK_MAX_Q + 1 && interval) acc[STDADK_GRID_WIDTH] += s;
  }
}

__global__ __launch_bounds__(kWave) void grid_score_split_kernel(const double *__restrict__ time_acc, int nT,
                                                                double *__restrict__ split_acc) {
  const int tid = threadIdx.x;
  if (tid >= GS_TV) return;
  const int c = tid / 3, v = tid % 3;
  double s = 0.0;
  for (int ti = 0; ti < nT; ++ti) s += time_acc[((size_t)c * nT + ti) * 3 + v];
  split_acc[(size_t)c * STDADK_GRID_SLOTS + (v == 0 ? STDADK_GRID_SSE : (v == 1 ? STDADK_GRID_SAE : STDADK_GRID_N))] += s;
}

}  // namespace stdadk

using namespace stdadk;

extern "C" size_t stdadk_grid_score_workspace_bytes(int64_t S, int64_t nT) {
  if (!grid_sizes_ok(S, nT)) return 0;
  const int64_t nblk = grid_score_blocks(S);
  return (size_t)nblk * (size_t)((nT > 0 ? nT : 1) * GS_TV + GS_XV) * sizeof(double);
}

extern "C" int stdadk_grid_score_f32(const float *y_pred, const float *z, const uint8_t *split, int64_t S, int64_t nT,
                                     int32_t Q, int32_t metric_col, const float *taus_host, int32_t lo_col,
                                     int32_t hi_col, double *split_acc, double *site_acc, double *time_acc,
                                     void *workspace, size_t workspace_bytes, stdadk_stream_t stream) {
  STDADK_REQUIRE(S >= 0 && nT >= 0, STDADK_E_ARG, "grid_score: negative size");
  if (S == 0 || nT == 0) return 0;
  STDADK_REQUIRE(y_pred && z && split_acc && site_acc && time_acc && workspace, STDADK_E_ARG,
                 "grid_score: NULL pointer");
  if (int rc = check_grid_args("grid_score", S, nT, Q, metric_col, lo_col, hi_col, workspace, workspace_bytes,
                               stdadk_grid_score_workspace_bytes(S, nT), "stdadk_grid_score_workspace_bytes"))
    return rc;
  const int nblk = (int)grid_score_blocks(S);
  GridScoreArgs a;
  a.yp = y_pred; a.z = z; a.split = split;
  a.S = (int)S; a.nT = (int)nT; a.mcol = metric_col; a.lo = lo_col; a.hi = hi_col;
  fill_taus(a.tau, taus_host, Q);
  a.site_acc = site_acc;
  a.tpart = (double *)workspace;
  a.xpart = a.tpart + (size_t)nblk * nT * GS_TV;
  hipStream_t st = (hipStream_t)stream;
  STDADK_LAUNCH_FOR_Q(Q, grid_score_kernel, dim3((unsigned)nblk), dim3(GS_T), 0, st, a);
  STDADK_CHECK_LAUNCH("grid_score");
  STDADK_LAUNCH(grid_score_time_kernel, dim3((unsigned)nT + 1), dim3(GS_T), 0, st, (const double *)a.tpart,
                (const double *)a.xpart, nblk, (int)nT, Q, lo_col >= 0 ? 1 : 0, time_acc, split_acc);
  STDADK_CHECK_LAUNCH("grid_score_time");
  STDADK_LAUNCH(grid_score_split_kernel, dim3(1), dim3(kWave), 0, st, (const double *)time_acc, (int)nT, split_acc);
  STDADK_CHECK_LAUNCH("grid_score_split");
  return 0;
}
