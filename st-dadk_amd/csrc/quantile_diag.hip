// Quantile diagnostics of a site x time prediction grid (stdadk_quantile_diag_f32, see include/stdadk.h): reliability,
// the PIT histogram over a row's own quantile ladder, crossings and their depth, CRPS and interval membership of one
// chunk of nT time slices of predictions [nT*S][Q] against the field z [nT][S] and the split codes, as float64 sums
// per split, per (split, site) and per (split, time).  The shape is grid_score.hip's -- three launches:
//   quantile_diag_kernel        one thread owns a SITE (lanes run along s) and walks the chunk's slices in time order.
//                               What is new is the number of sums: 3Q + 6 per split.  Most of them are COUNTS of a
//                               predicate, and a wave's count of a predicate is popcount(ballot & the split's ballot):
//                               scalar work on wave-uniform values, no per-lane register.  The 3Q counts per split
//                               that nothing else yields (BELOW, PIT, PAIR) are kept for the whole chunk in TWO
//                               vector registers, one counter per LANE (v_writelane puts an entry's popcount into the
//                               counter's lane of a staging register, one vector add per entry accumulates all of them),
//                               and leave through an ordinary store of those lanes.  Per-lane doubles are kept only
//                               for DEPTH1, DEPTH2 (4 x 2, chunk-long) and the site's crps (4); the site's three
//                               counts are per-lane integers, exact, added to the stored doubles at the end.  Per
//                               slice the (n, crps, cross_rows, inside) of every split leave as one partial per
//                               (workgroup, slice) through LDS tiles of QD_TT slices, as grid_score_kernel's do.
//   quantile_diag_time_kernel   workgroup ti < nT: the partials of slice ti over the workgroups, fixed order, into the
//                               workspace's time sums and ASSIGNED to time_acc when there is one; workgroup nT: the
//                               chunk-long partials (counts, depths), added into split_acc.
//   quantile_diag_split_kernel  N, CRPS, CROSS_ROWS, INSIDE of every split = the chunk's time sums added over its
//                               slices, added into split_acc.
// Every predicate and term is formed in double from operands converted to double, every operation rounded once (no
// contraction into fused multiply-adds: the terms are the bits a float64 restatement gives); no atomics anywhere: the
// same call on the same data gives the same bits.  Reads 4Q + 5 bytes per grid entry.
#include "grid_reduce.h"
#include "loss.h"

namespace stdadk {

constexpr int QD_TT = 16;                      // slices per LDS tile
constexpr int QD_TV = 16;                      // values per slice: 4 splits x (n, crps, cross_rows, inside)
constexpr int QD_K = 3 * STDADK_MAX_Q;         // chunk-long wave counts per split: BELOW[MAX_Q], PIT[MAX_Q + 1], PAIR[MAX_Q - 1]
constexpr int QD_KB = 0, QD_KP = STDADK_MAX_Q, QD_KX = 2 * STDADK_MAX_Q + 1;
constexpr int QD_X = QD_K + 2;                 // chunk-long values per split: the counts, depth1, depth2
constexpr int QD_XV = 4 * QD_X;
static_assert(GS_W == 4 && QD_TT % 8 == 0 && QD_TT * QD_TV <= GS_T && QD_XV <= GS_T, "quantile_diag_kernel's LDS hand-over");
static_assert(2 * QD_K <= kWave, "two splits' counters share one register's lanes");
static_assert(QD_TT * QD_TV >= QD_XV, "the chunk-long values reuse the tile");
static_assert(STDADK_QD_BELOW + STDADK_MAX_Q == STDADK_QD_PIT && STDADK_QD_PIT + STDADK_MAX_Q + 1 == STDADK_QD_CROSS_ROWS &&
                  STDADK_QD_PAIR + STDADK_MAX_Q - 1 == STDADK_QD_DEPTH1 && STDADK_QD_INSIDE < STDADK_QD_SLOTS,
              "per-split slots");

struct QuantileDiagArgs {
  const float *yp, *z;
  const uint8_t *split;
  int S, nT, lo, hi;
  float tau[STDADK_MAX_Q];
  double *site_acc, *tpart, *xpart;
};

// the count `v` (wave-uniform: a popcount of ballots, an SGPR the scalar unit wrote) into the lane of counter k of split
// c: splits 0, 1 in stage[0], splits 2, 3 in stage[1].  v_writelane_b32 has no builtin; the statement's operands are
// its whole effect, and an SGPR written by the scalar unit needs no wait state before it.
#define STDADK_QD_PUT(c, k, v)                                                   \
  asm("v_writelane_b32 %0, %1, %2"                                               \
      : "+v"(stage[(c) >> 1])                                                    \
      : "s"((int)(v)), "n"(((c) & 1) * QD_K + (k)))

template <int Q>
__global__ __launch_bounds__(GS_T) void quantile_diag_kernel(QuantileDiagArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[QD_TT][GS_W][QD_TV];
  constexpr int QD_U = Q <= 4 ? 8 : 4;  // slices whose loads are issued together (registers: QD_U * (Q + 2))
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int s = blockIdx.x * GS_T + tid;
  const bool live = s < a.S;            // the threads past the last site stay in every wave sum, adding nothing
  const bool interval = a.lo >= 0;
  const bool sites = live && a.site_acc;
  const double scale = 2.0 / (double)Q;
  double scr[4], d1[4], d2[4];
  uint32_t sn[4], sx[4], si[4];
  int cnt[2] = {0, 0}, stage[2] = {0, 0};   // every entry rewrites the same lanes of stage; the others stay 0
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    scr[c] = sites ? a.site_acc[((size_t)c * a.S + s) * 4 + 1] : 0.0;
    d1[c] = d2[c] = 0.0;
    sn[c] = sx[c] = si[c] = 0u;
  }
  for (int t0 = 0; t0 < a.nT; t0 += QD_TT) {
    const int nt = a.nT - t0 < QD_TT ? a.nT - t0 : QD_TT;
#pragma unroll
    for (int u0 = 0; u0 < QD_TT; u0 += QD_U) {
      if (u0 >= nt) break;
      float zf[QD_U], p[QD_U][Q];
      int code[QD_U];
#pragma unroll
      for (int u = 0; u < QD_U; ++u) {
        const bool on = live && u0 + u < nt;
        const size_t row = (size_t)(t0 + u0 + u) * a.S + s;
        zf[u] = on ? a.z[row] : __builtin_nanf("");
        code[u] = on && a.split ? (int)a.split[row] : 0;
#pragma unroll
        for (int q = 0; q < Q; ++q) p[u][q] = on ? a.yp[row * Q + q] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < QD_U; ++u) {
        if (u0 + u >= nt) break;
        const bool ok = zf[u] - zf[u] == 0.f;            // finite: NaN and +-inf count nowhere
        uint64_t mc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) mc[c] = __ballot(ok && code[u] == c);
        const double zd = (double)zf[u];
        double pd[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) pd[q] = (double)p[u][q];
        int rank = 0;                                    // #{q : p_q < z}
        double ck = 0.0;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const uint64_t b = __ballot(zd <= pd[q]);
#pragma unroll
          for (int c = 0; c < 4; ++c) STDADK_QD_PUT(c, QD_KB + q, __builtin_popcountll(b & mc[c]));
          rank += pd[q] < zd ? 1 : 0;
          const double r = check_elem((double)a.tau[q], pd[q], zd);
          ck = q == 0 ? r : ck + r;
        }
        const double crps = scale * ck;
#pragma unroll
        for (int j = 0; j <= Q; ++j) {
          const uint64_t b = __ballot(rank == j);
#pragma unroll
          for (int c = 0; c < 4; ++c) STDADK_QD_PUT(c, QD_KP + j, __builtin_popcountll(b & mc[c]));
        }
        bool cross = false;
        double e1 = 0.0, e2 = 0.0;
#pragma unroll
        for (int q = 0; q + 1 < Q; ++q) {
          const bool x = pd[q] > pd[q + 1];
          const uint64_t b = __ballot(x);
#pragma unroll
          for (int c = 0; c < 4; ++c) STDADK_QD_PUT(c, QD_KX + q, __builtin_popcountll(b & mc[c]));
          cross = cross || x;
          const double g = fmax(0.0, pd[q] - pd[q + 1]);
          const double g2 = g * g;
          e1 = q == 0 ? g : e1 + g;
          e2 = q == 0 ? g2 : e2 + g2;
        }
        cnt[0] += stage[0];
        cnt[1] += stage[1];
        double pl = pd[0], ph = pd[0];
#pragma unroll
        for (int q = 1; q < Q; ++q) {
          pl = q == a.lo ? pd[q] : pl;
          ph = q == a.hi ? pd[q] : ph;
        }
        const bool inside = interval && pl <= zd && zd <= ph;
        const uint64_t bx = __ballot(cross), bi = __ballot(inside);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool m = ok && code[u] == c;
          const double mcr = m ? crps : 0.0;
          d1[c] += m ? e1 : 0.0;
          d2[c] += m ? e2 : 0.0;
          scr[c] += mcr;
          sn[c] += m ? 1u : 0u;
          sx[c] += m && cross ? 1u : 0u;
          si[c] += m && inside ? 1u : 0u;
          const double w = wave_sum_f64(mcr);
          if (lane == 0) {
            red[u0 + u][wave][c * 4 + 0] = (double)__builtin_popcountll(mc[c]);
            red[u0 + u][wave][c * 4 + 1] = w;
            red[u0 + u][wave][c * 4 + 2] = (double)__builtin_popcountll(bx & mc[c]);
            red[u0 + u][wave][c * 4 + 3] = (double)__builtin_popcountll(bi & mc[c]);
          }
        }
      }
    }
    __syncthreads();
    if (tid < nt * QD_TV) {
      const int tl = tid / QD_TV, k = tid % QD_TV;
      a.tpart[((size_t)blockIdx.x * a.nT + t0 + tl) * QD_TV + k] =
          (red[tl][0][k] + red[tl][1][k]) + (red[tl][2][k] + red[tl][3][k]);
    }
    __syncthreads();
  }
  if (sites) {
    // the three counts are integers: adding them at once is adding them one by one
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double *acc = a.site_acc + ((size_t)c * a.S + s) * 4;
      acc[0] += (double)sn[c];
      acc[1] = scr[c];
      acc[2] += (double)sx[c];
      acc[3] += (double)si[c];
    }
  }
  double *xr = &red[0][0][0];           // [GS_W][QD_XV]
#pragma unroll
  for (int r = 0; r < 2; ++r)
    if (lane < 2 * QD_K) xr[wave * QD_XV + (2 * r + lane / QD_K) * QD_X + lane % QD_K] = (double)cnt[r];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double w1 = wave_sum_f64(d1[c]), w2 = wave_sum_f64(d2[c]);
    if (lane == 0) {
      xr[wave * QD_XV + c * QD_X + QD_K] = w1;
      xr[wave * QD_XV + c * QD_X + QD_K + 1] = w2;
    }
  }
  __syncthreads();
  if (tid < QD_XV)
    a.xpart[(size_t)blockIdx.x * QD_XV + tid] =
        (xr[tid] + xr[QD_XV + tid]) + (xr[2 * QD_XV + tid] + xr[3 * QD_XV + tid]);
}
#undef STDADK_QD_PUT

// tsum [nT][QD_TV]: the chunk's time sums in the workspace (time_acc may be NULL; the split sums are made of them)
__global__ __launch_bounds__(GS_T) void quantile_diag_time_kernel(const double *__restrict__ tpart,
                                                                 const double *__restrict__ xpart, int nblk, int nT,
                                                                 int Q, double *__restrict__ tsum,
                                                                 double *__restrict__ time_acc,
                                                                 double *__restrict__ split_acc) {
  __shared__ double red[GS_T];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < nT) {
    const int ti = blockIdx.x;
    const double s = sum_partials<QD_TV>(red, nblk, [&](int i) { return tpart + ((size_t)i * nT + ti) * QD_TV; });
    if (tid < QD_TV) {
      tsum[(size_t)ti * QD_TV + tid] = s;
      if (time_acc) time_acc[((size_t)(tid / 4) * nT + ti) * 4 + tid % 4] = s;
    }
    return;
  }
  const double s = sum_partials<QD_XV>(red, nblk, [&](int i) { return xpart + (size_t)i * QD_XV; });
  if (tid < QD_XV) {
    const int c = tid / QD_X, j = tid % QD_X;
    double *acc = split_acc + (size_t)c * STDADK_QD_SLOTS;
    if (j >= QD_KB && j < QD_KB + Q) acc[STDADK_QD_BELOW + j - QD_KB] += s;
    if (j >= QD_KP && j <= QD_KP + Q) acc[STDADK_QD_PIT + j - QD_KP] += s;
    if (j >= QD_KX && j < QD_KX + Q - 1) acc[STDADK_QD_PAIR + j - QD_KX] += s;
    if (j == QD_K) acc[STDADK_QD_DEPTH1] += s;
    if (j == QD_K + 1) acc[STDADK_QD_DEPTH2] += s;
  }
}

__global__ __launch_bounds__(kWave) void quantile_diag_split_kernel(const double *__restrict__ tsum, int nT,
                                                                   double *__restrict__ split_acc) {
  const int tid = threadIdx.x;
  if (tid >= QD_TV) return;
  const int c = tid / 4, v = tid % 4;
  double s = 0.0;
  for (int ti = 0; ti < nT; ++ti) s += tsum[(size_t)ti * QD_TV + tid];
  const int slot = v == 0 ? STDADK_QD_N : (v == 1 ? STDADK_QD_CRPS : (v == 2 ? STDADK_QD_CROSS_ROWS : STDADK_QD_INSIDE));
  split_acc[(size_t)c * STDADK_QD_SLOTS + slot] += s;
}

}  // namespace stdadk

using namespace stdadk;

extern "C" size_t stdadk_quantile_diag_workspace_bytes(int64_t S, int64_t nT) {
  if (!grid_sizes_ok(S, nT)) return 0;
  const int64_t nblk = grid_score_blocks(S), slices = nT > 0 ? nT : 1;
  return ((size_t)nblk * (size_t)(slices * QD_TV + QD_XV) + (size_t)slices * QD_TV) * sizeof(double);
}

extern "C" int stdadk_quantile_diag_f32(const float *y_pred, const float *z, const uint8_t *split, int64_t S, int64_t nT,
                                        int32_t Q, const float *taus_host, int32_t lo_col, int32_t hi_col,
                                        double *split_acc, double *site_acc, double *time_acc, void *workspace,
                                        size_t workspace_bytes, stdadk_stream_t stream) {
  STDADK_REQUIRE(S >= 0 && nT >= 0, STDADK_E_ARG, "quantile_diag: negative size");
  if (S == 0 || nT == 0) return 0;
  STDADK_REQUIRE(y_pred && z && split_acc && workspace, STDADK_E_ARG, "quantile_diag: NULL pointer");
  if (int rc = check_grid_args("quantile_diag", S, nT, Q, 0, lo_col, hi_col, workspace, workspace_bytes,
                               stdadk_quantile_diag_workspace_bytes(S, nT), "stdadk_quantile_diag_workspace_bytes"))
    return rc;
  const int nblk = (int)grid_score_blocks(S);
  QuantileDiagArgs a;
  a.yp = y_pred; a.z = z; a.split = split;
  a.S = (int)S; a.nT = (int)nT; a.lo = lo_col; a.hi = hi_col;
  fill_taus(a.tau, taus_host, Q);
  a.site_acc = site_acc;
  a.tpart = (double *)workspace;
  a.xpart = a.tpart + (size_t)nblk * nT * QD_TV;
  double *tsum = a.xpart + (size_t)nblk * QD_XV;
  hipStream_t st = (hipStream_t)stream;
  STDADK_LAUNCH_FOR_Q(Q, quantile_diag_kernel, dim3((unsigned)nblk), dim3(GS_T), 0, st, a);
  STDADK_CHECK_LAUNCH("quantile_diag");
  STDADK_LAUNCH(quantile_diag_time_kernel, dim3((unsigned)nT + 1), dim3(GS_T), 0, st, (const double *)a.tpart,
                (const double *)a.xpart, nblk, (int)nT, Q, tsum, time_acc, split_acc);
  STDADK_CHECK_LAUNCH("quantile_diag_time");
  STDADK_LAUNCH(quantile_diag_split_kernel, dim3(1), dim3(kWave), 0, st, (const double *)tsum, (int)nT, split_acc);
  STDADK_CHECK_LAUNCH("quantile_diag_split");
  return 0;
}
