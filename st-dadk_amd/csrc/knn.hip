// Neighbour tables (stdadk_knn_f32, stdadk_knn_apply_f32; see include/stdadk.h): the k nearest sources of every target
// in the total order (d2, source index), brute force, and a table applied to a field (nearest value, inverse-distance
// weighting).  Launches:
//   knn_search_kernel<KT>  grid (target tiles x slices, G source spans), KN_Q waves per workgroup: a thread owns ONE
//                        target of the tile of KN_MT and, with its wave, a quarter of every chunk of KN_SC staged sources
//                        of the workgroup's span (coordinates as doubles and the slice's source flag; every lane of a
//                        wave reads the same source: broadcast reads, no bank conflict; a non-source is skipped by the
//                        whole wave), in source order.  Its best-KT list (KT = k rounded up to 1, 2, 4, 8 or 16) stays in
//                        registers: fully unrolled compare-and-shift insertion, static indices only, no scratch.  A wave
//                        meets its sources in index order, so `strictly smaller` keeps equal distances at the lower
//                        index.  After the walk waves 1 .. 3 hand their lists over in LDS and wave 0 merges them in the
//                        total order; the workgroup writes the row itself (G == 1) or one partial row per span.
//   knn_finish_kernel<KT>  (G != 1) a thread per (slice, target) merges the spans' partial rows in span order -- later
//                        spans hold higher indices, so strictly smaller is again the total order -- and ASSIGNS the row;
//                        G == 0 (no source) writes the neutral rows.
//   knn_apply_kernel     a thread per (slice, target), sequential over the first k entries of its row.
// SPAN RULE (the sizes alone).  chunks = ceil(S / KN_SC), groups = ceil(M / KN_MT) x nM.  The sources are cut when the
// groups alone are fewer than KN_FILL = 1024 workgroups (four per compute unit): want = min(ceil(KN_FILL / groups),
// KN_MAX_SPANS, chunks), a span holds per = ceil(chunks / want) whole chunks and G = ceil(chunks / per): no span is
// empty.  One tile of one slice is cut from S = KN_SC + 1 = 257 on; 1024 groups or more are never cut.
// A distance is carried as its KEY, the bit pattern of the double read as an unsigned integer: d2 is a sum of two
// squares, never negative and never -0, so unsigned order is numeric order, +inf included; every NaN pattern is at or
// above KN_EMPTY (the pattern after +inf's), the key of an empty slot, and `key < last` lets no NaN in.  The order being
// total, the partition over waves and spans cannot change a bit of the answer.  The key, the list insertion, the row
// store and the argument checks live in knn_common.h: knn_cells.hip returns the same table and shares them.
#include "knn_common.h"

namespace stdadk {

constexpr int KN_Q = 4;                        // waves per workgroup
constexpr int KN_T = KN_Q * kWave;             // threads per workgroup
constexpr int KN_MT = kWave;                   // targets per workgroup (one per lane)
constexpr int KN_SC = 256;                     // sources staged per LDS chunk
constexpr int KN_SQ = KN_SC / KN_Q;            // a wave's share of a staged chunk
constexpr int KN_FILL = 1024;                  // workgroups below which the sources are cut into spans
constexpr int KN_MAX_SPANS = 64;               // source spans (partial rows per target) at the most
static_assert(KN_SC == KN_T, "one staged source per thread");

struct KnnArgs {
  const float *q, *coords;
  const uint8_t *src;
  int M, S, tiles, k, exclude_self, G, span;   // span: sources per span, a whole number of chunks KN_SC
  long long rows;                              // nM * M
  u64 *part_key;                               // [G][rows][k]
  int *part_idx;                               // [G][rows][k]
  int *nbr_idx;
  double *nbr_d2;
};

// slot e of a finished list as the table holds it
__device__ __forceinline__ void knn_store(const KnnArgs &a, size_t at, u64 key, int ix) {
  knn_store_slot(a.nbr_idx, a.nbr_d2, at, key, ix);
}

template <int KT>
__global__ __launch_bounds__(KN_T) void knn_search_kernel(KnnArgs a) {
  __shared__ double sx[KN_SC], sy[KN_SC];
  __shared__ int sf[KN_SC];
  __shared__ u64 mk[KN_Q - 1][KT][KN_MT];
  __shared__ int mi[KN_Q - 1][KT][KN_MT];
  const int tid = threadIdx.x, lane = tid % kWave, w = tid / kWave, g = blockIdx.y;
  const int m = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const long long j = (long long)tile * KN_MT + lane;
  const bool mine = j < a.M;
  const double qx = mine ? (double)a.q[2 * (size_t)j] : 0.0, qy = mine ? (double)a.q[2 * (size_t)j + 1] : 0.0;
  const long long self = a.exclude_self ? j : -1;
  const uint8_t *flags = a.src ? a.src + (size_t)m * a.S : nullptr;
  u64 key[KT];
  int ix[KT];
#pragma unroll
  for (int e = 0; e < KT; ++e) {
    key[e] = KN_EMPTY;
    ix[e] = KN_NONE;
  }
  const long long s_begin = (long long)g * a.span;
  const long long s_end = s_begin + a.span < a.S ? s_begin + a.span : a.S;
  for (long long s0 = s_begin; s0 < s_end; s0 += KN_SC) {
    const int nv = (int)(s_end - s0 < KN_SC ? s_end - s0 : KN_SC);
    __syncthreads();
    if (tid < nv) {
      const size_t i = (size_t)(s0 + tid);
      sx[tid] = (double)a.coords[2 * i];
      sy[tid] = (double)a.coords[2 * i + 1];
      sf[tid] = flags ? flags[i] != 0 : 1;
    }
    __syncthreads();
    if (!mine) continue;
    const int e_end = (w + 1) * KN_SQ < nv ? (w + 1) * KN_SQ : nv;      // this wave's quarter of the chunk
    for (int e = w * KN_SQ; e < e_end; ++e) {
      if (!sf[e]) continue;                    // (the same for every lane)
      const u64 c = (u64)__double_as_longlong(sq_dist_f64(qx, qy, sx[e], sy[e]));
      if (c < key[KT - 1] && s0 + e != self) knn_insert<KT, false>(key, ix, c, (int)(s0 + e));
    }
  }
  if (w > 0) {
#pragma unroll
    for (int e = 0; e < KT; ++e) {
      mk[w - 1][e][lane] = key[e];
      mi[w - 1][e][lane] = ix[e];
    }
  }
  __syncthreads();
  if (!mine || w > 0) return;
  for (int v = 0; v < KN_Q - 1; ++v) {         // the other waves' lists, each ascending: (key, index) decides
#pragma unroll
    for (int e = 0; e < KT; ++e) {
      const u64 c = mk[v][e][lane];
      const int i = mi[v][e][lane];
      if (c < key[KT - 1] || (c == key[KT - 1] && i < ix[KT - 1])) knn_insert<KT, true>(key, ix, c, i);
    }
  }
  const size_t row = (size_t)m * a.M + (size_t)j;
  if (a.G == 1) {
#pragma unroll
    for (int e = 0; e < KT; ++e)
      if (e < a.k) knn_store(a, row * a.k + e, key[e], ix[e]);
  } else {
    const size_t at = ((size_t)g * a.rows + row) * a.k;
#pragma unroll
    for (int e = 0; e < KT; ++e)
      if (e < a.k) {
        a.part_key[at + e] = key[e];
        a.part_idx[at + e] = ix[e];
      }
  }
}

template <int KT>
__global__ __launch_bounds__(KN_T) void knn_finish_kernel(KnnArgs a) {
  const long long row = (long long)blockIdx.x * KN_T + threadIdx.x;
  if (row >= a.rows) return;
  u64 key[KT];
  int ix[KT];
#pragma unroll
  for (int e = 0; e < KT; ++e) {
    key[e] = KN_EMPTY;
    ix[e] = KN_NONE;
  }
  for (int g = 0; g < a.G; ++g) {              // span order: equal keys arrive in index order
    const size_t at = ((size_t)g * a.rows + (size_t)row) * a.k;
    for (int e = 0; e < a.k; ++e) {
      const u64 c = a.part_key[at + e];
      if (c < key[KT - 1]) knn_insert<KT, false>(key, ix, c, a.part_idx[at + e]);
    }
  }
#pragma unroll
  for (int e = 0; e < KT; ++e)
    if (e < a.k) knn_store(a, (size_t)row * a.k + e, key[e], ix[e]);
}

struct KnnApplyArgs {
  const int *nbr_idx;
  const double *nbr_d2;
  const float *z;
  float *nearest, *idw;
  int nM, M, k_tab, k, nT, S, power;
};

__global__ __launch_bounds__(KN_T) void knn_apply_kernel(KnnApplyArgs a) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * KN_T + threadIdx.x;
  if (r >= (long long)a.nT * a.M) return;
  const long long ti = r / a.M, j = r % a.M;
  const size_t row = ((size_t)(a.nM == 1 ? 0 : ti) * a.M + (size_t)j) * a.k_tab;
  const float *zs = a.z + (size_t)ti * a.S;
  int first = -1;
  bool zero = false, run = true;
  double num = 0.0, den = 0.0;
  for (int e = 0; e < a.k; ++e) {
    const int i = a.nbr_idx[row + e];
    if (i < 0 || i >= a.S) continue;           // the tail of a short row (and never a read outside z)
    const double d2 = a.nbr_d2[row + e];
    const double zv = (double)zs[i];
    if (first < 0) {
      first = i;
      zero = d2 == 0.0;
    }
    if (zero) {                                // the mean over the leading run of zero distances
      run = run && d2 == 0.0;
      if (run) {
        num += zv;
        den += 1.0;
      }
    } else {
      double wt = 1.0;
      switch (a.power) {
        case 1: wt = 1.0 / sqrt(d2); break;
        case 2: wt = 1.0 / d2; break;
        case 3: wt = 1.0 / (d2 * sqrt(d2)); break;
        case 4: wt = 1.0 / (d2 * d2); break;
        default: break;
      }
      const double t = wt * zv;
      num += t;
      den += wt;
    }
  }
  const float nan = __builtin_nanf("");
  if (a.nearest) a.nearest[r] = first < 0 ? nan : zs[first];
  if (a.idw) a.idw[r] = first < 0 ? nan : (float)(num / den);
}

// the source spans of the search (the rule of the head comment); no source, target or slice: no span
struct KnSpans {
  int64_t G, span;
};
static inline KnSpans knn_spans(int64_t M, int64_t S, int64_t nM) {
  const int64_t chunks = ceil_div(S, KN_SC);
  if (chunks == 0 || M == 0 || nM == 0) return KnSpans{0, KN_SC};
  int64_t want = ceil_div(KN_FILL, ceil_div(M, KN_MT) * nM);
  want = want < KN_MAX_SPANS ? want : KN_MAX_SPANS;
  want = want < chunks ? want : chunks;
  const int64_t per = ceil_div(chunks, want);
  return KnSpans{ceil_div(chunks, per), per * KN_SC};
}

}  // namespace stdadk

using namespace stdadk;

extern "C" size_t stdadk_knn_workspace_bytes(int64_t M, int64_t S, int64_t nM, int32_t k) {
  if (!knn_sizes_ok(M, S, nM, k)) return 0;
  const int64_t G = knn_spans(M, S, nM).G;
  const size_t need = G > 1 ? (size_t)G * (size_t)(nM * M) * k * (sizeof(u64) + sizeof(int)) : 0;
  return need > 8 ? align_up(need, 8) : 8;     // (never 0 for sizes that are accepted)
}

extern "C" int stdadk_knn_f32(const float *q, int64_t M, const float *coords, int64_t S, const uint8_t *src, int64_t nM,
                              int32_t k, int32_t exclude_self, int32_t *nbr_idx, double *nbr_d2, void *workspace,
                              size_t workspace_bytes, stdadk_stream_t stream) {
  if (int rc = knn_check_call("knn", q, M, coords, S, src, nM, k, exclude_self, nbr_idx, nbr_d2, workspace, workspace_bytes,
                              stdadk_knn_workspace_bytes(M, S, nM, k), "stdadk_knn_workspace_bytes"))
    return rc;
  if (M == 0 || nM == 0) return 0;

  const KnSpans sp = knn_spans(M, S, nM);
  KnnArgs a;
  a.q = q; a.coords = coords; a.src = src;
  a.M = (int)M; a.S = (int)S; a.tiles = (int)ceil_div(M, KN_MT); a.k = k; a.exclude_self = exclude_self;
  a.G = (int)sp.G; a.span = (int)sp.span;
  a.rows = nM * M;
  a.part_key = (u64 *)workspace;
  a.part_idx = (int *)((u64 *)workspace + (size_t)sp.G * (size_t)a.rows * k);
  a.nbr_idx = nbr_idx; a.nbr_d2 = nbr_d2;
  hipStream_t st = (hipStream_t)stream;
  const dim3 search((unsigned)(a.tiles * nM), (unsigned)sp.G), finish((unsigned)ceil_div(a.rows, KN_T));
#define STDADK_KNN_FOR_K(KT)                                                              \
  do {                                                                                    \
    if (sp.G > 0) {                                                                       \
      STDADK_LAUNCH(knn_search_kernel<KT>, search, dim3(KN_T), 0, st, a);                 \
      STDADK_CHECK_LAUNCH("knn_search");                                                  \
    }                                                                                     \
    if (sp.G != 1) {                                                                      \
      STDADK_LAUNCH(knn_finish_kernel<KT>, finish, dim3(KN_T), 0, st, a);                 \
      STDADK_CHECK_LAUNCH("knn_finish");                                                  \
    }                                                                                     \
  } while (0)
  if (k == 1)
    STDADK_KNN_FOR_K(1);
  else if (k == 2)
    STDADK_KNN_FOR_K(2);
  else if (k <= 4)
    STDADK_KNN_FOR_K(4);
  else if (k <= 8)
    STDADK_KNN_FOR_K(8);
  else
    STDADK_KNN_FOR_K(16);
#undef STDADK_KNN_FOR_K
  return 0;
}

extern "C" int stdadk_knn_apply_f32(const int32_t *nbr_idx, const double *nbr_d2, int64_t nM, int64_t M, int32_t k_tab,
                                    int32_t k, const float *z, int64_t nT, int64_t S, int32_t power, float *nearest,
                                    float *idw, stdadk_stream_t stream) {
  const int64_t lim = 1ll << 31;
  STDADK_REQUIRE(M >= 0 && S >= 0 && nT >= 0 && nM >= 0 && M < lim && S < lim && nT < lim && nM < lim, STDADK_E_ARG,
                 "knn_apply: M=%lld, S=%lld, nT=%lld, nM=%lld must be 0 .. 2^31-1", (long long)M, (long long)S,
                 (long long)nT, (long long)nM);
  STDADK_REQUIRE(nM == 1 || nM == nT, STDADK_E_ARG, "knn_apply: nM=%lld must be 1 or nT=%lld", (long long)nM, (long long)nT);
  STDADK_REQUIRE(k_tab >= 1 && k_tab <= STDADK_KNN_MAX_K && k >= 1 && k <= k_tab, STDADK_E_ARG,
                 "knn_apply: k_tab=%d outside 1..%d or k=%d outside 1..k_tab", k_tab, STDADK_KNN_MAX_K, k);
  STDADK_REQUIRE(power >= 0 && power <= 4, STDADK_E_ARG, "knn_apply: power=%d outside 0..4", power);
  STDADK_REQUIRE(nT * M < lim && nT * S < lim && nM * M * k_tab < lim, STDADK_E_SHAPE,
                 "knn_apply: nT*M, nT*S and nM*M*k_tab must stay below 2^31 (nT=%lld, M=%lld, S=%lld, nM=%lld, k_tab=%d)",
                 (long long)nT, (long long)M, (long long)S, (long long)nM, k_tab);
  const bool any = nT > 0 && M > 0;
  STDADK_REQUIRE(!any || (nbr_idx && nbr_d2 && (S == 0 || z)), STDADK_E_ARG, "knn_apply: NULL pointer");
  STDADK_REQUIRE(!any || nearest || idw, STDADK_E_ARG, "knn_apply: nearest and idw both NULL");
  STDADK_REQUIRE((reinterpret_cast<uintptr_t>(nbr_d2) & 7) == 0, STDADK_E_ALIGN, "knn_apply: nbr_d2 not 8-byte aligned");
  STDADK_REQUIRE(((reinterpret_cast<uintptr_t>(nbr_idx) | reinterpret_cast<uintptr_t>(z) |
                   reinterpret_cast<uintptr_t>(nearest) | reinterpret_cast<uintptr_t>(idw)) & 3) == 0,
                 STDADK_E_ALIGN, "knn_apply: nbr_idx, z, nearest or idw not 4-byte aligned");
  const size_t n_tab = (size_t)(nM * M) * k_tab, n_out = (size_t)(nT * M) * sizeof(float);
  const ByteRange out[2] = {{nearest, nearest ? n_out : 0}, {idw, idw ? n_out : 0}};
  const ByteRange in[3] = {{nbr_idx, n_tab * sizeof(int32_t)}, {nbr_d2, n_tab * sizeof(double)},
                           {z, (size_t)(nT * S) * sizeof(float)}};
  if (int rc = check_no_alias("knn_apply", out, in, "")) return rc;
  if (!any) return 0;
  KnnApplyArgs a;
  a.nbr_idx = nbr_idx; a.nbr_d2 = nbr_d2; a.z = z; a.nearest = nearest; a.idw = idw;
  a.nM = (int)nM; a.M = (int)M; a.k_tab = k_tab; a.k = k; a.nT = (int)nT; a.S = (int)S; a.power = power;
  STDADK_LAUNCH(knn_apply_kernel, dim3((unsigned)ceil_div(nT * M, KN_T)), dim3(KN_T), 0, (hipStream_t)stream, a);
  STDADK_CHECK_LAUNCH("knn_apply");
  return 0;
}
