// Local ordinary kriging on a neighbour table (stdadk_krige_weights_f64, stdadk_krige_apply_f32; see include/stdadk.h):
// per row of the table one symmetric system of at most 16 x 16, solved by Cholesky in a FIXED order, and the weights
// applied to a field with the kriging variance turned into Gaussian quantiles.  Launches:
//   krige_weights_kernel<W>  W = k rounded up to 1, 2, 4, 8 or 16 lanes per row, 64 / W rows per wave, KR_T / W per
//                        workgroup.  Lane e of a group owns entry e of the row: its index, its coordinates, and ROW e of
//                        the matrix, whole (both triangles), in registers.  An entry that does not count, or that
//                        coincides with an earlier one, holds an identity row (diagonal 1, everything else and both right
//                        sides 0): it changes no bit of the others, so no system is compacted.  The factorisation is
//                        right-looking: in step c every lane divides its element of column c by the pivot lane c
//                        broadcasts, then takes L_bc from lane b (b > c) and subtracts L_ac L_bc from its element b --
//                        element (a, b) so meets its products in increasing c.  Both triangles are updated (the same
//                        operands, the same bits), which saves every select; lane c keeps the column it receives as
//                        U_c[b] = L_bc, the row of L^T it needs going back.  The two right sides (1 and k) ride along.
//                        Broadcasts are __shfl over the W lanes of the group: no LDS, no barrier.  Rows whose groups
//                        share a wave are independent.
//   krige_apply_kernel   a thread per (slice, target), sequential over the first k entries of its row.
// Contraction is off: a fused multiply-add would round once where the contract rounds the product, then the difference.
#include "f64_block.h"

namespace stdadk {

constexpr int KR_T = 256;                      // threads per workgroup
static_assert(STDADK_KNN_MAX_K == 16, "group widths 1, 2, 4, 8, 16");

struct KrigeArgs {
  const int *nbr_idx;
  const double *nbr_d2;
  const float *coords;
  double *w, *var;
  long long rows;                              // nM * M
  int k_tab, k, S, model;
  double nugget, psill, range;
};

// the model's correlation of the distance sqrt(d2): 1 at 0, falling to 0
__device__ __forceinline__ double krige_rho(int model, double d2, double range) {
#pragma clang fp contract(off)
  const double d = sqrt(d2);
  const double r = d / range;
  const double r2 = r * r;
  if (model == STDADK_KRIGE_SPHERICAL) {
    const double t = 0.5 * r2;
    const double u = 1.5 - t;
    const double v = r * u;
    return d < range ? 1.0 - v : (d >= range ? 0.0 : __builtin_nan(""));
  }
  if (model == STDADK_KRIGE_GAUSSIAN) return exp(-r2);
  return exp(-r);
}

template <int W>
__device__ __forceinline__ double group_get(double v, int src) {
  return W == 1 ? v : __shfl(v, src, W);
}
template <int W>
__device__ __forceinline__ int group_get(int v, int src) {
  return W == 1 ? v : __shfl(v, src, W);
}

template <int W>
__global__ __launch_bounds__(KR_T) void krige_weights_kernel(KrigeArgs a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, e = tid % W;
  const long long row = ((long long)blockIdx.x * KR_T + tid) / W;
  const bool live = row < a.rows && e < a.k;
  const unsigned long long group = (W == 64 ? ~0ull : ((1ull << W) - 1)) << ((tid % kWave) / W * W);

  int idx = -1;
  double d0 = 0.0;
  if (live) {
    idx = a.nbr_idx[(size_t)row * a.k_tab + e];
    d0 = a.nbr_d2[(size_t)row * a.k_tab + e];
  }
  const bool counts = idx >= 0 && idx < a.S;   // (never a read outside coords)
  const double x = counts ? (double)a.coords[2 * (size_t)idx] : 0.0, y = counts ? (double)a.coords[2 * (size_t)idx + 1] : 0.0;

  // coincident entries: the group of the FIRST earlier entry at squared distance exactly 0 (that entry is a first member)
  double dd[W];
  int rep = e;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const double xc = group_get<W>(x, c), yc = group_get<W>(y, c);
    const int cc = group_get<W>((int)counts, c);
    dd[c] = sq_dist_f64(x, y, xc, yc);
    if (counts && cc && c < e && dd[c] == 0.0 && rep == e) rep = c;
  }
  const bool act = counts && rep == e;         // this lane holds an unknown of the system
  int members = 0;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const int rc = group_get<W>(rep, c), cc = group_get<W>((int)counts, c);
    members += (cc && rc == e) ? 1 : 0;
  }

  double s[W], u_row[W];
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const int ac = group_get<W>((int)act, c);
    const double cov = a.psill * krige_rho(a.model, dd[c], a.range);
    s[c] = (act && ac) ? cov : 0.0;
    u_row[c] = 0.0;
  }
  const double own = a.nugget / (double)(members > 0 ? members : 1);
#pragma unroll
  for (int c = 0; c < W; ++c)
    if (c == e) s[c] = act ? a.psill + own : 1.0;
  const double kk = act ? a.psill * krige_rho(a.model, d0, a.range) : 0.0;
  double r1 = act ? 1.0 : 0.0, rk = kk, pivot = 1.0;
  bool bad = false;

  // K = L L^T, and L y = (1, k) with it
#pragma unroll
  for (int c = 0; c < W; ++c) {
    if (e == c && act && !(s[c] > 0.0 && s[c] < __builtin_inf())) bad = true;
    const double p = group_get<W>(sqrt(s[c]), c);
    if (e == c) pivot = p;
    const double l = s[c] / p;                 // L_ec on the lanes e > c
    const double y1 = r1 / p, yk = rk / p;     // y_c on lane c
    const double y1c = group_get<W>(y1, c), ykc = group_get<W>(yk, c);
    const double t1 = l * y1c, tk = l * ykc;
    r1 = e > c ? r1 - t1 : (e == c ? y1 : r1);
    rk = e > c ? rk - tk : (e == c ? yk : rk);
#pragma unroll
    for (int b = c + 1; b < W; ++b) {
      const double lb = group_get<W>(l, b);    // L_bc
      const double t = l * lb;
      s[b] = s[b] - t;                         // (lanes e <= c: dead values, never read again)
      u_row[b] = e == c ? lb : u_row[b];
    }
  }
  // L^T x = y: the unknowns become known from the last one down, and are subtracted in that order
#pragma unroll
  for (int c = W - 1; c >= 0; --c) {
    const double x1 = r1 / pivot, xk = rk / pivot;
    const double x1c = group_get<W>(x1, c), xkc = group_get<W>(xk, c);
    const double t1 = u_row[c] * x1c, tk = u_row[c] * xkc;
    r1 = e < c ? r1 - t1 : (e == c ? x1 : r1);
    rk = e < c ? rk - tk : (e == c ? xk : rk);
  }
  double su = 0.0, sv = 0.0;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    su += group_get<W>(r1, c);
    sv += group_get<W>(rk, c);
  }
  const double mu = (sv - 1.0) / su;
  const double tm = mu * r1;
  const double wt = rk - tm;
  const double prod = act ? wt * kk : 0.0;
  double swk = 0.0;
#pragma unroll
  for (int c = 0; c < W; ++c) swk += group_get<W>(prod, c);
  const double c00 = a.nugget + a.psill;
  const double v0 = c00 - swk;
  double var = v0 - mu;

  const bool singular = (__ballot(bad) & group) != 0, some = (__ballot(act) & group) != 0;
  const double w_rep = group_get<W>(wt, rep);
  const int m_rep = group_get<W>(members, rep);
  double w_out = counts ? w_rep / (double)(m_rep > 0 ? m_rep : 1) : 0.0;
  const double nan = __builtin_nan("");
  if (singular) {
    w_out = nan;
    var = nan;
  } else if (!some) {
    var = nan;
  }
  if (live) {
    a.w[(size_t)row * a.k + e] = w_out;
    if (e == 0) a.var[row] = var;
  }
}

struct KrigeApplyArgs {
  const int *nbr_idx;
  const double *w, *var;
  const float *z;
  float *out;
  int nM, M, k_tab, k, nT, S, Q;
  long long ldo;
  double zq[STDADK_KRIGE_MAX_COLS];
};

__global__ __launch_bounds__(KR_T) void krige_apply_kernel(KrigeApplyArgs a) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * KR_T + threadIdx.x;
  if (r >= (long long)a.nT * a.M) return;
  const long long ti = r / a.M, j = r % a.M;
  const size_t trow = (size_t)(a.nM == 1 ? 0 : ti) * a.M + (size_t)j;
  const float *zs = a.z + (size_t)ti * a.S;
  double p = 0.0;
  for (int e = 0; e < a.k; ++e) {
    const int i = a.nbr_idx[trow * a.k_tab + e];
    if (i < 0 || i >= a.S) continue;           // the tail of a short row (and never a read outside z)
    const double t = a.w[trow * a.k + e] * (double)zs[i];
    p += t;
  }
  const double var = a.var[trow];
  const double sd = sqrt(var > 0.0 ? var : 0.0);
  const bool none = var != var;
  float *o = a.out + (size_t)r * a.ldo;
#pragma unroll
  for (int c = 0; c < STDADK_KRIGE_MAX_COLS; ++c)
    if (c < a.Q) {
      const double t = a.zq[c] * sd;
      o[c] = none ? __builtin_nanf("") : (float)(p + t);
    }
}

static inline bool finite_f64(double v) { return v == v && v - v == 0.0; }

}  // namespace stdadk

using namespace stdadk;

extern "C" int stdadk_krige_weights_f64(const int32_t *nbr_idx, const double *nbr_d2, int64_t nM, int64_t M, int32_t k_tab,
                                        int32_t k, const float *coords, int64_t S, int32_t model, double nugget,
                                        double psill, double range, double *w, double *var, stdadk_stream_t stream) {
  const int64_t lim = 1ll << 31;
  STDADK_REQUIRE(M >= 0 && S >= 0 && nM >= 0 && M < lim && S < lim && nM < lim, STDADK_E_ARG,
                 "krige_weights: M=%lld, S=%lld, nM=%lld must be 0 .. 2^31-1", (long long)M, (long long)S, (long long)nM);
  STDADK_REQUIRE(k_tab >= 1 && k_tab <= STDADK_KNN_MAX_K && k >= 1 && k <= k_tab, STDADK_E_ARG,
                 "krige_weights: k_tab=%d outside 1..%d or k=%d outside 1..k_tab", k_tab, STDADK_KNN_MAX_K, k);
  STDADK_REQUIRE(model >= STDADK_KRIGE_EXPONENTIAL && model <= STDADK_KRIGE_GAUSSIAN, STDADK_E_ARG,
                 "krige_weights: model=%d outside 0..2", model);
  STDADK_REQUIRE(finite_f64(nugget) && finite_f64(psill) && finite_f64(range) && nugget >= 0.0 && psill >= 0.0 &&
                     nugget + psill > 0.0 && finite_f64(nugget + psill) && range > 0.0,
                 STDADK_E_ARG, "krige_weights: nugget=%g, psill=%g must be finite, >= 0 and not both 0, range=%g finite and > 0",
                 nugget, psill, range);
  STDADK_REQUIRE(nM * M < lim && nM * M * k_tab < lim, STDADK_E_SHAPE,
                 "krige_weights: nM*M*k_tab = %lld x %lld x %d must stay below 2^31", (long long)nM, (long long)M, k_tab);
  const bool rows = M > 0 && nM > 0;
  STDADK_REQUIRE(!rows || (nbr_idx && nbr_d2 && w && var && (S == 0 || coords)), STDADK_E_ARG, "krige_weights: NULL pointer");
  STDADK_REQUIRE(((reinterpret_cast<uintptr_t>(nbr_d2) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(var)) & 7) == 0,
                 STDADK_E_ALIGN, "krige_weights: nbr_d2, w or var not 8-byte aligned");
  STDADK_REQUIRE(((reinterpret_cast<uintptr_t>(nbr_idx) | reinterpret_cast<uintptr_t>(coords)) & 3) == 0, STDADK_E_ALIGN,
                 "krige_weights: nbr_idx or coords not 4-byte aligned");
  const size_t n_rows = (size_t)(nM * M), n_tab = n_rows * k_tab;
  const ByteRange out[2] = {{w, n_rows * k * sizeof(double)}, {var, n_rows * sizeof(double)}};
  const ByteRange in[3] = {{nbr_idx, n_tab * sizeof(int32_t)}, {nbr_d2, n_tab * sizeof(double)},
                           {coords, (size_t)S * 2 * sizeof(float)}};
  if (int rc = check_no_alias("krige_weights", out, in, "")) return rc;
  if (!rows) return 0;

  KrigeArgs a;
  a.nbr_idx = nbr_idx; a.nbr_d2 = nbr_d2; a.coords = coords; a.w = w; a.var = var;
  a.rows = nM * M; a.k_tab = k_tab; a.k = k; a.S = (int)S; a.model = model;
  a.nugget = nugget; a.psill = psill; a.range = range;
  hipStream_t st = (hipStream_t)stream;
#define STDADK_KRIGE_FOR_W(W)                                                                              \
  do {                                                                                                     \
    STDADK_LAUNCH(krige_weights_kernel<W>, dim3((unsigned)ceil_div(a.rows, KR_T / W)), dim3(KR_T), 0, st, a); \
    STDADK_CHECK_LAUNCH("krige_weights");                                                                  \
  } while (0)
  if (k == 1)
    STDADK_KRIGE_FOR_W(1);
  else if (k == 2)
    STDADK_KRIGE_FOR_W(2);
  else if (k <= 4)
    STDADK_KRIGE_FOR_W(4);
  else if (k <= 8)
    STDADK_KRIGE_FOR_W(8);
  else
    STDADK_KRIGE_FOR_W(16);
#undef STDADK_KRIGE_FOR_W
  return 0;
}

extern "C" int stdadk_krige_apply_f32(const int32_t *nbr_idx, const double *w, const double *var, int64_t nM, int64_t M,
                                      int32_t k_tab, int32_t k, const float *z, int64_t nT, int64_t S,
                                      const double *zq_host, int32_t Q, float *out, int64_t ldo, stdadk_stream_t stream) {
  const int64_t lim = 1ll << 31;
  STDADK_REQUIRE(M >= 0 && S >= 0 && nT >= 0 && nM >= 0 && M < lim && S < lim && nT < lim && nM < lim, STDADK_E_ARG,
                 "krige_apply: M=%lld, S=%lld, nT=%lld, nM=%lld must be 0 .. 2^31-1", (long long)M, (long long)S,
                 (long long)nT, (long long)nM);
  STDADK_REQUIRE(nM == 1 || nM == nT, STDADK_E_ARG, "krige_apply: nM=%lld must be 1 or nT=%lld", (long long)nM, (long long)nT);
  STDADK_REQUIRE(k_tab >= 1 && k_tab <= STDADK_KNN_MAX_K && k >= 1 && k <= k_tab, STDADK_E_ARG,
                 "krige_apply: k_tab=%d outside 1..%d or k=%d outside 1..k_tab", k_tab, STDADK_KNN_MAX_K, k);
  STDADK_REQUIRE(Q >= 1 && Q <= STDADK_KRIGE_MAX_COLS && ldo >= Q && ldo < lim && zq_host, STDADK_E_ARG,
                 "krige_apply: Q=%d outside 1..%d, ldo=%lld below Q (or 2^31 and above), or zq_host NULL", Q,
                 STDADK_KRIGE_MAX_COLS, (long long)ldo);
  for (int c = 0; c < Q; ++c)
    STDADK_REQUIRE(finite_f64(zq_host[c]), STDADK_E_ARG, "krige_apply: zq_host[%d] is not finite", c);
  STDADK_REQUIRE(nT * M < lim && nT * S < lim && nM * M * k_tab < lim, STDADK_E_SHAPE,
                 "krige_apply: nT*M, nT*S and nM*M*k_tab must stay below 2^31 (nT=%lld, M=%lld, S=%lld, nM=%lld, k_tab=%d)",
                 (long long)nT, (long long)M, (long long)S, (long long)nM, k_tab);
  const bool any = nT > 0 && M > 0;
  STDADK_REQUIRE(!any || (nbr_idx && w && var && out && (S == 0 || z)), STDADK_E_ARG, "krige_apply: NULL pointer");
  STDADK_REQUIRE(((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(var)) & 7) == 0, STDADK_E_ALIGN,
                 "krige_apply: w or var not 8-byte aligned");
  STDADK_REQUIRE(((reinterpret_cast<uintptr_t>(nbr_idx) | reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(out)) & 3) == 0,
                 STDADK_E_ALIGN, "krige_apply: nbr_idx, z or out not 4-byte aligned");
  const size_t n_rows = (size_t)(nM * M);
  const ByteRange outs[1] = {{out, any ? ((size_t)(nT * M - 1) * (size_t)ldo + Q) * sizeof(float) : 0}};
  const ByteRange in[4] = {{nbr_idx, n_rows * k_tab * sizeof(int32_t)}, {w, n_rows * k * sizeof(double)},
                           {var, n_rows * sizeof(double)}, {z, (size_t)(nT * S) * sizeof(float)}};
  if (int rc = check_no_alias("krige_apply", outs, in, "")) return rc;
  if (!any) return 0;
  KrigeApplyArgs a;
  a.nbr_idx = nbr_idx; a.w = w; a.var = var; a.z = z; a.out = out;
  a.nM = (int)nM; a.M = (int)M; a.k_tab = k_tab; a.k = k; a.nT = (int)nT; a.S = (int)S; a.Q = Q; a.ldo = ldo;
  for (int c = 0; c < STDADK_KRIGE_MAX_COLS; ++c) a.zq[c] = c < Q ? zq_host[c] : 0.0;
  STDADK_LAUNCH(krige_apply_kernel, dim3((unsigned)ceil_div(nT * M, KR_T)), dim3(KR_T), 0, (hipStream_t)stream, a);
  STDADK_CHECK_LAUNCH("krige_apply");
  return 0;
}
