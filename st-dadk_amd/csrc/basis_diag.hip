// Basis diagnostics (stdadk_basis_diag_f32, stdadk_group_norms_f32; see include/stdadk.h): what did the BASIS do?  A
// sites x knots pair reduction on the live knot tables -- per knot the training data inside its support, per site and
// level the knots that cover it -- and the float64 group norms of the first Linear's basis columns.  Three launches
// for the pair reduction, every pair evaluated once per direction:
//   basis_knot_kernel    grid (knot tiles of BD_KT, G site spans), BD_Q waves per workgroup: a thread owns ONE knot
//                        of the tile and, with its wave, every BD_Q-th sub-chunk of BD_SC sites of the workgroup's
//                        span, in site order: BD_Q x BD_SC sites are staged in LDS at a time as doubles (every lane
//                        of a wave reads the same site: broadcast reads, no bank conflict; a site without weight is
//                        skipped by the whole wave).  Its seven values stay in registers; after the walk the waves'
//                        values of a knot are added in wave order and the workgroup leaves one partial row [7][Ks]
//                        per span.
//   basis_knot_finish_kernel  a thread per knot adds the spans' rows in span order (NEAR2: their minimum) and ASSIGNS
//                        knot_acc [Ks][7].
//   basis_site_kernel    grid (site tiles of BD_ST, levels), BD_Q waves per workgroup: a thread owns ONE site of the
//                        tile and, with its wave, a quarter of every chunk of BD_KC staged knots of the level (centre,
//                        R2 and the radius scale as doubles, broadcast reads), in knot order; the waves' values of a
//                        site are added in wave order and ASSIGNED to site_acc [S][n_levels][3]: no partial rows on
//                        this side.
// Every value is formed in double from operands converted to double, every operation rounded once (contraction off);
// the in-support decision d2 < R2 is an exact comparison.  Every sum is of non-negative weights times phi in [0, 1] in
// an order fixed by the sizes alone; no atomics: the same call gives the same bits.  The walk is double-precision
// vector issue, not memory.
#include "f64_block.h"
#include "grid_reduce.h"

namespace stdadk {

constexpr int BD_Q = 4;                        // waves per workgroup of either direction: BD_Q x 64 threads
constexpr int BD_T = BD_Q * kWave;             // threads per workgroup
constexpr int BD_KT = kWave;                   // knots per workgroup of the knot direction (one per lane)
constexpr int BD_SC = 64;                      // sites per sub-chunk: a wave's share of a staged block
constexpr int BD_SS = BD_Q * BD_SC;            // sites staged per LDS block of the knot direction
constexpr int BD_MAX_SPANS = 16;               // site spans (partial rows per knot) at the most
constexpr int BD_ST = kWave;                   // sites per workgroup of the site direction (one per lane)
constexpr int BD_KC = 256;                     // knots staged per LDS chunk of the site direction
constexpr int BD_KQ = BD_KC / BD_Q;            // a wave's share of a staged chunk of knots
constexpr int BD_NV = STDADK_BD_KNOT_SLOTS;    // values per knot
static_assert(BD_NV == 7 && STDADK_BD_K_N == 0 && STDADK_BD_K_W == 1 && STDADK_BD_K_SPHI == 2 && STDADK_BD_K_SPHI2 == 3 &&
              STDADK_BD_K_SV == 4 && STDADK_BD_K_WV == 5 && STDADK_BD_K_NEAR2 == 6, "slots of a knot");
static_assert(STDADK_BD_SITE_SLOTS == 3 && STDADK_BD_S_COVER == 0 && STDADK_BD_S_SPHI == 1 && STDADK_BD_S_NEAR2 == 2,
              "slots of a site and level");
static_assert(BD_SS == BD_T && BD_KC == BD_T, "both directions stage one site / knot per thread");

__host__ __device__ static inline double basis_cal(int basis) {
  return basis == STDADK_BASIS_GAUSSIAN ? 0.223477 : basis == STDADK_BASIS_TRIANGULAR ? 0.654714 : 1.0;
}

// phi(r) in double with the formulas of basis.h (no fused multiply-add: a host restatement forms the same products)
template <int BASIS>
__device__ __forceinline__ double basis_eval_f64(double r) {
#pragma clang fp contract(off)
  if (BASIS == STDADK_BASIS_WENDLAND) {
    r = r < 1.0 ? r : 1.0;
    const double om = 1.0 - r;
    const double om2 = om * om;
    const double om6 = om2 * om2 * om2;
    const double poly = (35.0 * r + 18.0) * r + 3.0;
    return om6 * poly / 3.0;
  } else if (BASIS == STDADK_BASIS_GAUSSIAN) {
    return exp(-0.5 * r * r);
  } else {
    const double om = 1.0 - r;
    return om > 0.0 ? om : 0.0;
  }
}

// the two scales of knot k: den = bw cal (r = sqrt(d2) / den) and R2 = (den rho)^2
struct BdKnot {
  double den, R2;
};
__device__ __forceinline__ BdKnot bd_knot(float bw, double cal, double rho) {
#pragma clang fp contract(off)
  const double den = (double)bw * cal;
  const double s = den * rho;
  return BdKnot{den, s * s};
}

struct BasisDiagArgs {
  const float *centers, *bw, *coords;
  const double *w, *v;
  int Ks, S, n_levels, G, span;                // span: sites per span, a whole number of sub-chunks BD_SC
  double rho;
  double *part;                                // [G][BD_NV][Ks]
  double *knot_acc, *site_acc;
  int level_off[STDADK_MAX_LEVELS + 1];        // knots of level l: level_off[l] .. level_off[l + 1] - 1
};

template <int BASIS>
__global__ __launch_bounds__(BD_T) void basis_knot_kernel(BasisDiagArgs a) {
#pragma clang fp contract(off)
  __shared__ double sx[BD_SS], sy[BD_SS], sw[BD_SS], sv[BD_SS], sm[BD_SS];
  __shared__ double fold[BD_NV][BD_Q][BD_KT];
  const int tid = threadIdx.x, g = blockIdx.y, lane = tid % kWave, q = tid / kWave;
  const long long k = (long long)blockIdx.x * BD_KT + lane;
  const bool mine = k < a.Ks;
  double cx = 0.0, cy = 0.0;
  BdKnot kn{1.0, 0.0};
  if (mine) {
    cx = (double)a.centers[2 * (size_t)k];
    cy = (double)a.centers[2 * (size_t)k + 1];
    kn = bd_knot(a.bw[k], basis_cal(BASIS), a.rho);
  }
  double n = 0.0, W = 0.0, sphi = 0.0, sphi2 = 0.0, SV = 0.0, WV = 0.0, near2 = __builtin_inf();
  const long long s_begin = (long long)g * a.span;
  const long long s_end = s_begin + a.span < a.S ? s_begin + a.span : a.S;
  for (long long s0 = s_begin; s0 < s_end; s0 += BD_SS) {
    const int nv = (int)(s_end - s0 < BD_SS ? s_end - s0 : BD_SS);
    __syncthreads();
    if (tid < nv) {
      const size_t i = (size_t)(s0 + tid);
      sx[tid] = (double)a.coords[2 * i];
      sy[tid] = (double)a.coords[2 * i + 1];
      const double wi = a.w ? a.w[i] : 1.0;
      sw[tid] = (wi - wi == 0.0 && wi > 0.0) ? wi : 0.0;      // finite and > 0: the site counts; else 0 = skipped
      const double vi = a.v ? a.v[i] : 0.0;
      const bool vf = a.v && vi - vi == 0.0;
      sv[tid] = vf ? vi : 0.0;
      sm[tid] = vf ? 1.0 : 0.0;
    }
    __syncthreads();
    if (!mine) continue;
    const int q_end = (q + 1) * BD_SC < nv ? (q + 1) * BD_SC : nv;      // this wave's sub-chunk of the block
    for (int e = q * BD_SC; e < q_end; ++e) {
      const double wi = sw[e];
      if (!(wi > 0.0)) continue;               // (the same for every lane)
      const double d2 = sq_dist_f64(sx[e], sy[e], cx, cy);
      near2 = d2 < near2 ? d2 : near2;
      if (d2 < kn.R2) {
        const double phi = basis_eval_f64<BASIS>(sqrt(d2) / kn.den);
        const double t = wi * phi;
        n += 1.0;
        W += wi;
        sphi += t;
        sphi2 += t * phi;
        if (sm[e] != 0.0) {
          SV += t * sv[e];
          WV += t;
        }
      }
    }
  }
  fold[0][q][lane] = n;
  fold[1][q][lane] = W;
  fold[2][q][lane] = sphi;
  fold[3][q][lane] = sphi2;
  fold[4][q][lane] = SV;
  fold[5][q][lane] = WV;
  fold[6][q][lane] = near2;
  __syncthreads();
  if (mine && q == 0) {                        // the waves' values in wave order
    double *row = a.part + (size_t)g * BD_NV * a.Ks + (size_t)k;
#pragma unroll
    for (int v = 0; v < BD_NV; ++v) {
      double r = fold[v][0][lane];
#pragma unroll
      for (int w = 1; w < BD_Q; ++w) {
        const double x = fold[v][w][lane];
        if (v == STDADK_BD_K_NEAR2)
          r = x < r ? x : r;
        else
          r += x;
      }
      row[(size_t)v * a.Ks] = r;
    }
  }
}

// knot_acc [Ks][7] = the spans' partial rows added in span order, NEAR2 their minimum; G = 0 (no site): the neutral row
__global__ __launch_bounds__(BD_T) void basis_knot_finish_kernel(const double *__restrict__ part, int G, int Ks,
                                                                double *__restrict__ knot_acc) {
  const long long k = (long long)blockIdx.x * BD_T + threadIdx.x;
  if (k >= Ks) return;
  double s[BD_NV];
#pragma unroll
  for (int v = 0; v < BD_NV; ++v) s[v] = v == STDADK_BD_K_NEAR2 ? __builtin_inf() : 0.0;
  for (int g = 0; g < G; ++g) {
    const double *row = part + (size_t)g * BD_NV * Ks + (size_t)k;
#pragma unroll
    for (int v = 0; v < BD_NV; ++v) {
      const double x = row[(size_t)v * Ks];
      if (v == STDADK_BD_K_NEAR2)
        s[v] = x < s[v] ? x : s[v];
      else
        s[v] += x;
    }
  }
#pragma unroll
  for (int v = 0; v < BD_NV; ++v) knot_acc[(size_t)k * BD_NV + v] = s[v];
}

template <int BASIS>
__global__ __launch_bounds__(BD_T) void basis_site_kernel(BasisDiagArgs a) {
#pragma clang fp contract(off)
  __shared__ double kx[BD_KC], ky[BD_KC], kden[BD_KC], kR2[BD_KC];
  __shared__ double fold[STDADK_BD_SITE_SLOTS][BD_Q][BD_ST];
  const int tid = threadIdx.x, l = blockIdx.y, lane = tid % kWave, q = tid / kWave;
  const long long i = (long long)blockIdx.x * BD_ST + lane;
  const bool mine = i < a.S;
  const double x = mine ? (double)a.coords[2 * (size_t)i] : 0.0, y = mine ? (double)a.coords[2 * (size_t)i + 1] : 0.0;
  const int k_begin = a.level_off[l], k_end = a.level_off[l + 1];
  double cover = 0.0, sphi = 0.0, near2 = __builtin_inf();
  for (int k0 = k_begin; k0 < k_end; k0 += BD_KC) {
    const int nv = k_end - k0 < BD_KC ? k_end - k0 : BD_KC;
    __syncthreads();
    if (tid < nv) {
      const size_t k = (size_t)(k0 + tid);
      const BdKnot kn = bd_knot(a.bw[k], basis_cal(BASIS), a.rho);
      kx[tid] = (double)a.centers[2 * k];
      ky[tid] = (double)a.centers[2 * k + 1];
      kden[tid] = kn.den;
      kR2[tid] = kn.R2;
    }
    __syncthreads();
    if (!mine) continue;
    const int q_end = (q + 1) * BD_KQ < nv ? (q + 1) * BD_KQ : nv;      // this wave's quarter of the chunk
    for (int e = q * BD_KQ; e < q_end; ++e) {
      const double d2 = sq_dist_f64(x, y, kx[e], ky[e]);
      near2 = d2 < near2 ? d2 : near2;
      if (d2 < kR2[e]) {
        cover += 1.0;
        sphi += basis_eval_f64<BASIS>(sqrt(d2) / kden[e]);
      }
    }
  }
  fold[STDADK_BD_S_COVER][q][lane] = cover;
  fold[STDADK_BD_S_SPHI][q][lane] = sphi;
  fold[STDADK_BD_S_NEAR2][q][lane] = near2;
  __syncthreads();
  if (mine && q == 0) {                        // the waves' values in wave order
    double *row = a.site_acc + ((size_t)i * a.n_levels + l) * STDADK_BD_SITE_SLOTS;
#pragma unroll
    for (int w = 1; w < BD_Q; ++w) {
      cover += fold[STDADK_BD_S_COVER][w][lane];
      sphi += fold[STDADK_BD_S_SPHI][w][lane];
      const double m = fold[STDADK_BD_S_NEAR2][w][lane];
      near2 = m < near2 ? m : near2;
    }
    row[STDADK_BD_S_COVER] = cover;
    row[STDADK_BD_S_SPHI] = sphi;
    row[STDADK_BD_S_NEAR2] = near2;
  }
}

// the site spans of the knot direction: G spans of `span` sites, span a whole number of BD_SC chunks, G <= BD_MAX_SPANS
// and no span empty; S = 0: no span
struct BdSpans {
  int64_t G, span;
};
static inline BdSpans basis_diag_spans(int64_t S) {
  const int64_t chunks = ceil_div(S, BD_SC);
  if (chunks == 0) return BdSpans{0, BD_SC};
  const int64_t per = ceil_div(chunks, BD_MAX_SPANS);
  return BdSpans{ceil_div(chunks, per), per * BD_SC};
}

static inline bool basis_diag_sizes_ok(int64_t S, int64_t Ks) {
  return S >= 0 && Ks >= 0 && S < (1ll << 31) && Ks < (1ll << 31);
}

// sum of squares of group j = col0 + blockIdx.x * 256 + thread: a COLUMN of W0 (H, ld), rows in order
__global__ __launch_bounds__(GS_T) void group_norms_cols_kernel(const float *__restrict__ W0, long long ld, int H, int col0,
                                                               int n, double *__restrict__ out) {
#pragma clang fp contract(off)
  const long long j = (long long)blockIdx.x * GS_T + threadIdx.x;
  if (j >= n) return;
  double s = 0.0;
  for (int h = 0; h < H; ++h) {
    const double x = (double)W0[(size_t)h * ld + col0 + j];
    s += x * x;
  }
  out[j] = s;
}

// sum of squares of group j = col0 + blockIdx.x * GS_W + wave: a ROW of W0^T (D, ld); a lane adds the terms h = lane,
// lane + 64, ... in order, the lanes' sums go through the fixed tree of wave_sum_f64
__global__ __launch_bounds__(GS_T) void group_norms_rows_kernel(const float *__restrict__ W0T, long long ld, int H, int col0,
                                                               int n, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x % kWave;
  const long long j = (long long)blockIdx.x * GS_W + threadIdx.x / kWave;
  if (j >= n) return;                          // (the whole wave)
  const float *row = W0T + (size_t)(col0 + j) * ld;
  double s = 0.0;
  for (int h = lane; h < H; h += kWave) {
    const double x = (double)row[h];
    s += x * x;
  }
  s = wave_sum_f64(s);
  if (lane == 0) out[j] = s;
}

}  // namespace stdadk

using namespace stdadk;

extern "C" size_t stdadk_basis_diag_workspace_bytes(int64_t S, int64_t Ks) {
  if (!basis_diag_sizes_ok(S, Ks)) return 0;
  const size_t need = (size_t)basis_diag_spans(S).G * BD_NV * (size_t)Ks * sizeof(double);
  return need > 8 ? need : 8;                  // (never 0 for sizes that are accepted)
}

extern "C" int stdadk_basis_diag_f32(const float *s_centers, const float *s_bw, int64_t Ks, int32_t basis,
                                     const int64_t *level_sizes_host, int32_t n_levels, const float *coords, int64_t S,
                                     const double *w, const double *v, double rho, double *knot_acc, double *site_acc,
                                     void *workspace, size_t workspace_bytes, stdadk_stream_t stream) {
  STDADK_REQUIRE(basis_diag_sizes_ok(S, Ks), STDADK_E_ARG, "basis_diag: S=%lld, Ks=%lld must be 0 .. 2^31-1",
                 (long long)S, (long long)Ks);
  STDADK_REQUIRE(basis == STDADK_BASIS_WENDLAND || basis == STDADK_BASIS_GAUSSIAN || basis == STDADK_BASIS_TRIANGULAR,
                 STDADK_E_ARG, "basis_diag: unknown basis kind %d", basis);
  STDADK_REQUIRE(n_levels >= 1 && n_levels <= STDADK_MAX_LEVELS, STDADK_E_ARG, "basis_diag: n_levels=%d outside 1..%d",
                 n_levels, STDADK_MAX_LEVELS);
  STDADK_REQUIRE(level_sizes_host, STDADK_E_ARG, "basis_diag: NULL pointer");
  int64_t sum = 0;
  for (int l = 0; l < n_levels; ++l) {
    STDADK_REQUIRE(level_sizes_host[l] >= 0 && level_sizes_host[l] <= Ks, STDADK_E_ARG,
                   "basis_diag: level_sizes[%d]=%lld outside 0..Ks=%lld", l, (long long)level_sizes_host[l], (long long)Ks);
    sum += level_sizes_host[l];
  }
  STDADK_REQUIRE(sum == Ks, STDADK_E_ARG, "basis_diag: level_sizes sum to %lld, Ks=%lld", (long long)sum, (long long)Ks);
  STDADK_REQUIRE(rho > 0.0 && rho - rho == 0.0, STDADK_E_ARG, "basis_diag: rho=%g must be finite and > 0", rho);
  STDADK_REQUIRE((Ks == 0 || (s_centers && s_bw && knot_acc)) && (S == 0 || (coords && site_acc)) && workspace,
                 STDADK_E_ARG, "basis_diag: NULL pointer");
  STDADK_REQUIRE(((reinterpret_cast<uintptr_t>(knot_acc) | reinterpret_cast<uintptr_t>(site_acc) |
                   reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(v)) & 7) == 0,
                 STDADK_E_ALIGN, "basis_diag: knot_acc, site_acc, w or v not 8-byte aligned");
  if (int rc = check_workspace("basis_diag", workspace, workspace_bytes, stdadk_basis_diag_workspace_bytes(S, Ks),
                               "stdadk_basis_diag_workspace_bytes"))
    return rc;
  const ByteRange out[3] = {{knot_acc, (size_t)Ks * BD_NV * sizeof(double)},
                            {site_acc, (size_t)S * n_levels * STDADK_BD_SITE_SLOTS * sizeof(double)},
                            {workspace, workspace_bytes}};
  const ByteRange in[5] = {{s_centers, (size_t)Ks * 2 * sizeof(float)},
                           {s_bw, (size_t)Ks * sizeof(float)},
                           {coords, (size_t)S * 2 * sizeof(float)},
                           {w, w ? (size_t)S * sizeof(double) : 0},
                           {v, v ? (size_t)S * sizeof(double) : 0}};
  if (int rc = check_no_alias("basis_diag", out, in, "")) return rc;

  const BdSpans sp = basis_diag_spans(S);
  BasisDiagArgs a;
  a.centers = s_centers; a.bw = s_bw; a.coords = coords; a.w = w; a.v = v;
  a.Ks = (int)Ks; a.S = (int)S; a.n_levels = n_levels; a.G = (int)sp.G; a.span = (int)sp.span;
  a.rho = rho;
  a.part = (double *)workspace; a.knot_acc = knot_acc; a.site_acc = site_acc;
  a.level_off[0] = 0;
  for (int l = 0; l < STDADK_MAX_LEVELS; ++l)
    a.level_off[l + 1] = a.level_off[l] + (l < n_levels ? (int)level_sizes_host[l] : 0);
  hipStream_t st = (hipStream_t)stream;
  const unsigned knot_tiles = (unsigned)ceil_div(Ks, BD_KT), site_tiles = (unsigned)ceil_div(S, BD_ST);
#define STDADK_BD_FOR_BASIS(kern, grid, block)                                            \
  switch (basis) {                                                                        \
    case STDADK_BASIS_WENDLAND:                                                           \
      STDADK_LAUNCH(kern<STDADK_BASIS_WENDLAND>, grid, block, 0, st, a);                  \
      break;                                                                              \
    case STDADK_BASIS_GAUSSIAN:                                                           \
      STDADK_LAUNCH(kern<STDADK_BASIS_GAUSSIAN>, grid, block, 0, st, a);                  \
      break;                                                                              \
    default:                                                                              \
      STDADK_LAUNCH(kern<STDADK_BASIS_TRIANGULAR>, grid, block, 0, st, a);                \
      break;                                                                              \
  }
  if (Ks > 0) {
    if (sp.G > 0) {
      STDADK_BD_FOR_BASIS(basis_knot_kernel, dim3(knot_tiles, (unsigned)sp.G), dim3(BD_T));
      STDADK_CHECK_LAUNCH("basis_knot");
    }
    STDADK_LAUNCH(basis_knot_finish_kernel, dim3((unsigned)ceil_div(Ks, BD_T)), dim3(BD_T), 0, st,
                  (const double *)workspace, (int)sp.G, (int)Ks, knot_acc);
    STDADK_CHECK_LAUNCH("basis_knot_finish");
  }
  if (S > 0) {
    STDADK_BD_FOR_BASIS(basis_site_kernel, dim3(site_tiles, (unsigned)n_levels), dim3(BD_T));
    STDADK_CHECK_LAUNCH("basis_site");
  }
#undef STDADK_BD_FOR_BASIS
  return 0;
}

extern "C" int stdadk_group_norms_f32(const float *W0, int64_t ld, int32_t transposed, int32_t H, int64_t col0, int64_t n,
                                      double *out, stdadk_stream_t stream) {
  STDADK_REQUIRE(H >= 1 && col0 >= 0 && n >= 0 && col0 + n < (1ll << 31), STDADK_E_ARG,
                 "group_norms: H=%d, col0=%lld, n=%lld: H >= 1, col0 >= 0, n >= 0, col0 + n < 2^31", H, (long long)col0,
                 (long long)n);
  STDADK_REQUIRE(transposed == 0 || transposed == 1, STDADK_E_ARG, "group_norms: transposed=%d must be 0 or 1", transposed);
  STDADK_REQUIRE(ld >= (transposed ? (int64_t)H : col0 + n) && ld < (1ll << 31), STDADK_E_ARG,
                 "group_norms: ld=%lld shorter than a row of %lld values", (long long)ld,
                 (long long)(transposed ? (int64_t)H : col0 + n));
  if (n == 0) return 0;
  STDADK_REQUIRE(W0 && out, STDADK_E_ARG, "group_norms: NULL pointer");
  STDADK_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, STDADK_E_ALIGN, "group_norms: out not 8-byte aligned");
  const size_t floats = transposed ? (size_t)(col0 + n - 1) * ld + H : (size_t)(H - 1) * ld + col0 + n;
  const ByteRange o[1] = {{out, (size_t)n * sizeof(double)}};
  const ByteRange in[1] = {{W0, floats * sizeof(float)}};
  if (int rc = check_no_alias("group_norms", o, in, "")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (transposed)
    STDADK_LAUNCH(group_norms_rows_kernel, dim3((unsigned)ceil_div(n, GS_W)), dim3(GS_T), 0, st, W0, (long long)ld, (int)H,
                  (int)col0, (int)n, out);
  else
    STDADK_LAUNCH(group_norms_cols_kernel, dim3((unsigned)ceil_div(n, GS_T)), dim3(GS_T), 0, st, W0, (long long)ld, (int)H,
                  (int)col0, (int)n, out);
  STDADK_CHECK_LAUNCH("group_norms");
  return 0;
}
