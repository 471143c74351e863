// Empirical space-time variograms of field, prediction and residual on a site x time grid (stdadk_variogram_f32, see
// include/stdadk.h): for every time lag u, distance bin b and split c the count of site pairs (a = (t, i),
// b = (t + u, j)) and the float64 sums of (z_a - z_b)^2, (p_a - p_b)^2 and (r_a - r_b)^2, r = z - p.  Two launches:
//   variogram_kernel         grid (G, lags): a workgroup owns ONE lag and walks the tiles VG_E x VG_E of site pairs
//                            wg, wg + G, ... of that lag (u = 0: the upper triangle of tiles, i < j inside a diagonal
//                            tile; u > 0: every ordered tile, i = j included).  A thread owns one pair of the tile: it
//                            forms d2 and the bin ONCE (sq_dist_f64, exact comparisons against the squared edges), then
//                            walks the slices in time order with the two blocks' (z, p, code) of VG_TC slices staged in
//                            LDS ([nT][S] is contiguous along sites: spans of VG_E values), its 4 x (n, sz, sp, sr) in
//                            registers.  A tile whose pairs all miss the bins is skipped before anything is staged.
//                            After the walk the threads' sums go to LDS and the thread that OWNS (bin, split, slot)
//                            adds the sums of the pairs of its bin in thread order onto its running value (a register:
//                            ceil(16 n_bins / 256) <= 4 of them); after its last tile the workgroup leaves one partial
//                            row [n_bins][16].
//   variogram_finish_kernel  workgroup (b, u): the partial rows of lag u over the workgroups, fixed order (sum_partials),
//                            ASSIGNED to acc; lags past the grid's slices get zeros.
// Every term is formed in double from operands converted to double, every operation rounded once (contraction off: a
// term is the bits a float64 restatement gives), every sum is of non-negative terms in a fixed order; no atomics: the
// same call gives the same bits.  The walk is bound by vector issue, two fifths of it the split selects.
#include "f64_block.h"
#include "grid_reduce.h"

namespace stdadk {

constexpr int VG_E = 16;                       // sites per tile edge: VG_E x VG_E pairs = one per thread
constexpr int VG_TC = 64;                      // slices staged per LDS chunk
constexpr int VG_NV = 16;                      // values per bin: 4 splits x (n, sz, sp, sr)
constexpr int VG_MAX_BINS = STDADK_VG_MAX_BINS, VG_MAX_LAGS = STDADK_VG_MAX_LAGS;
constexpr int VG_ROUNDS = VG_MAX_BINS * VG_NV / GS_T;      // owned (bin, value) slots per thread
constexpr int VG_MAX_WG = 1024;                // workgroups per lag (partial rows per lag)
constexpr int VG_PAD = GS_T + 1;               // fold[v][thread]: a value's row, padded so that 16 rows hit 32 banks
static_assert(VG_E * VG_E == GS_T && VG_ROUNDS * GS_T == VG_MAX_BINS * VG_NV, "one pair per thread, whole owner rounds");
static_assert(GS_T % VG_NV == 0, "variogram_finish_kernel's sum_partials");
static_assert(STDADK_VG_N == 0 && STDADK_VG_SZ == 1 && STDADK_VG_SP == 2 && STDADK_VG_SR == 3, "slots of a bin");

struct VariogramArgs {
  const float *yp, *z, *coords;
  const uint8_t *split;
  long long ldy;
  int col, S, nT, n_bins, G;
  double *part;                                // [lags launched][G][n_bins][VG_NV]
  double edges2[VG_MAX_BINS + 1];
};

struct VgStage {                               // [side a / b][slice][site of the block]
  float z[2][VG_TC][VG_E], p[2][VG_TC][VG_E];
  int code[2][VG_TC][VG_E];
};
struct VgFold {
  double v[VG_NV][VG_PAD];
  int bin[GS_T];
};
union VgLds {
  VgStage st;
  VgFold fo;
};

// tile (ti, tj) number idx of lag u among nt x nt tiles: u > 0 row-major over all of them; u == 0 the pairs ti <= tj,
// idx = tj (tj + 1) / 2 + ti
struct VgTile {
  int ti, tj;
};
__device__ __forceinline__ VgTile vg_tile(long long idx, int u, int nt) {
  long long c = (long long)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
  while (c > 0 && c * (c + 1) / 2 > idx) --c;
  while ((c + 1) * (c + 2) / 2 <= idx) ++c;
  const long long full_i = idx / nt, full_j = idx % nt;
  return VgTile{(int)(u > 0 ? full_i : idx - c * (c + 1) / 2), (int)(u > 0 ? full_j : c)};
}

template <bool HAS_P>
__global__ __launch_bounds__(GS_T) void variogram_kernel(VariogramArgs a) {
#pragma clang fp contract(off)
  __shared__ VgLds lds;
  const int tid = threadIdx.x, ty = tid / VG_E, tx = tid % VG_E;
  const int u = blockIdx.y, wg = blockIdx.x;
  const int nt = (int)(((long long)a.S + VG_E - 1) / VG_E);
  const long long ntiles = u > 0 ? (long long)nt * nt : (long long)nt * (nt + 1) / 2;
  const int nTu = a.nT - u;                    // slices t with t + u inside the grid (the launch has u < nT)
  const int nslots = a.n_bins * VG_NV;
  double own[VG_ROUNDS];
#pragma unroll
  for (int r = 0; r < VG_ROUNDS; ++r) own[r] = 0.0;

  for (long long idx = wg; idx < ntiles; idx += a.G) {
    const VgTile tile = vg_tile(idx, u, nt);
    const int ti = tile.ti, tj = tile.tj;
    const long long i = (long long)ti * VG_E + ty, j = (long long)tj * VG_E + tx;      // (S + 15 may pass 31 bits)
    int bin = -1;
    if (i < a.S && j < a.S && (u > 0 || i < j)) {
      const double d2 = sq_dist_f64((double)a.coords[2 * (size_t)i], (double)a.coords[2 * (size_t)i + 1],
                                    (double)a.coords[2 * (size_t)j], (double)a.coords[2 * (size_t)j + 1]);
      int k = 0;                               // edges <= d2: strictly increasing, so bin = k - 1 when 1 <= k <= n_bins
      for (int b = 0; b <= a.n_bins; ++b) k += a.edges2[b] <= d2 ? 1 : 0;
      bin = k >= 1 && k <= a.n_bins ? k - 1 : -1;
    }
    const bool active = bin >= 0;
    // (a barrier: the owners of the last tile have read the fold before this tile stages over it)
    if (!__syncthreads_or(active ? 1 : 0)) continue;
    int n[4];
    double sz[4], sp[4], sr[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      n[c] = 0;
      sz[c] = sp[c] = sr[c] = 0.0;
    }
    for (int t0 = 0; t0 < nTu; t0 += VG_TC) {
      const int nv = nTu - t0 < VG_TC ? nTu - t0 : VG_TC;
      __syncthreads();
      for (int e = tid; e < nv * 2 * VG_E; e += GS_T) {
        const int tl = e / (2 * VG_E), side = (e / VG_E) & 1, sl = e % VG_E;
        const int row = t0 + tl + (side ? u : 0);
        const long long site = (long long)(side ? tj : ti) * VG_E + sl;
        float zf = 0.f, pf = 0.f;
        int code = 4 + side;                   // no value: 4 on side a, 5 on side b, so that the two never match
        if (site < a.S) {                      // row < nT: tl < nv <= nT - u - t0
          const size_t at = (size_t)row * a.S + site;
          zf = a.z[at];
          const int cd = a.split ? (int)a.split[at] : 0;
          if (zf - zf == 0.f && cd <= 3) code = cd;      // finite z and a code 0..3: the entry is counted
          if (HAS_P) pf = a.yp[at * (size_t)a.ldy + a.col];
        }
        lds.st.z[side][tl][sl] = zf;
        lds.st.p[side][tl][sl] = pf;
        lds.st.code[side][tl][sl] = code;
      }
      __syncthreads();
      if (active) {
#pragma unroll 4
        for (int tl = 0; tl < nv; ++tl) {
          const int ca = lds.st.code[0][tl][ty], cb = lds.st.code[1][tl][tx];
          const double za = (double)lds.st.z[0][tl][ty], zb = (double)lds.st.z[1][tl][tx];
          const double dz = za - zb;
          const double tz = dz * dz;
          double tp = 0.0, tr = 0.0;
          if (HAS_P) {
            const double pa = (double)lds.st.p[0][tl][ty], pb = (double)lds.st.p[1][tl][tx];
            const double dp = pa - pb;
            tp = dp * dp;
            const double ra = za - pa, rb = zb - pb;
            const double dr = ra - rb;
            tr = dr * dr;
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const bool m = ca == c && cb == c;
            n[c] += m ? 1 : 0;
            sz[c] += m ? tz : 0.0;
            if (HAS_P) {
              sp[c] += m ? tp : 0.0;
              sr[c] += m ? tr : 0.0;
            }
          }
        }
      }
    }
    __syncthreads();                           // every walk is over: the fold takes the staging's place
    lds.fo.bin[tid] = bin;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      lds.fo.v[c * 4 + 0][tid] = (double)n[c];
      lds.fo.v[c * 4 + 1][tid] = sz[c];
      lds.fo.v[c * 4 + 2][tid] = sp[c];
      lds.fo.v[c * 4 + 3][tid] = sr[c];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VG_ROUNDS; ++r) {
      if (r * GS_T >= nslots) break;
      const int o = r * GS_T + tid, b = o / VG_NV, v = o % VG_NV;      // (b >= n_bins matches no pair: adds zeros)
      double s = own[r];
      for (int q = 0; q < GS_T; ++q) s += lds.fo.bin[q] == b ? lds.fo.v[v][q] : 0.0;
      own[r] = s;
    }
  }
  double *row = a.part + ((size_t)u * a.G + wg) * nslots;
#pragma unroll
  for (int r = 0; r < VG_ROUNDS; ++r) {
    const int o = r * GS_T + tid;
    if (o < nslots) row[o] = own[r];
  }
}

// acc [4][n_lags][n_bins][4] = the partial rows of (lag u, bin b) added in workgroup order; nrows = 0 past `lags_run`
__global__ __launch_bounds__(GS_T) void variogram_finish_kernel(const double *__restrict__ part, int G, int lags_run,
                                                               int n_bins, int n_lags, double *__restrict__ acc) {
  __shared__ double red[GS_T];
  const int b = blockIdx.x, u = blockIdx.y, tid = threadIdx.x;
  const int nrows = u < lags_run ? G : 0;
  const double s = sum_partials<VG_NV>(
      red, nrows, [&](int i) { return part + (((size_t)u * G + i) * n_bins + b) * VG_NV; });
  if (tid < VG_NV) acc[(((size_t)(tid / 4) * n_lags + u) * n_bins + b) * 4 + tid % 4] = s;
}

// workgroups per lag: one per tile of the full square of tiles, VG_MAX_WG at the most, at least one
static inline int64_t variogram_blocks(int64_t S) {
  const int64_t nt = ceil_div(S > 0 ? S : 1, VG_E);
  return nt >= 32 ? VG_MAX_WG : nt * nt;       // 32 x 32 = VG_MAX_WG
}
static_assert(VG_MAX_WG == 32 * 32, "variogram_blocks");

}  // namespace stdadk

using namespace stdadk;

extern "C" size_t stdadk_variogram_workspace_bytes(int64_t S, int64_t nT, int32_t n_bins, int32_t n_lags) {
  if (!grid_sizes_ok(S, nT) || n_bins < 1 || n_bins > VG_MAX_BINS || n_lags < 1 || n_lags > VG_MAX_LAGS) return 0;
  return (size_t)variogram_blocks(S) * (size_t)n_lags * (size_t)n_bins * VG_NV * sizeof(double);
}

extern "C" int stdadk_variogram_f32(const float *y_pred, int64_t ldy, int32_t col, const float *z, const uint8_t *split,
                                    const float *coords, int64_t S, int64_t nT, const double *edges2_host,
                                    int32_t n_bins, int32_t n_lags, double *acc, void *workspace,
                                    size_t workspace_bytes, stdadk_stream_t stream) {
  STDADK_REQUIRE(S >= 0 && nT >= 0, STDADK_E_ARG, "variogram: negative size");
  STDADK_REQUIRE(n_bins >= 1 && n_bins <= VG_MAX_BINS, STDADK_E_ARG, "variogram: n_bins=%d outside 1..%d", n_bins,
                 VG_MAX_BINS);
  STDADK_REQUIRE(n_lags >= 1 && n_lags <= VG_MAX_LAGS, STDADK_E_ARG, "variogram: n_lags=%d outside 1..%d", n_lags,
                 VG_MAX_LAGS);
  STDADK_REQUIRE(edges2_host && acc && workspace, STDADK_E_ARG, "variogram: NULL pointer");
  STDADK_REQUIRE(edges2_host[0] >= 0.0, STDADK_E_ARG, "variogram: edges2[0]=%g must be >= 0", edges2_host[0]);
  for (int b = 0; b < n_bins; ++b)             // (a NaN edge fails the comparison)
    STDADK_REQUIRE(edges2_host[b] < edges2_host[b + 1], STDADK_E_ARG,
                   "variogram: edges2 must be strictly increasing (edges2[%d]=%g, edges2[%d]=%g)", b, edges2_host[b],
                   b + 1, edges2_host[b + 1]);
  STDADK_REQUIRE(!y_pred || (col >= 0 && col < ldy), STDADK_E_ARG, "variogram: col=%d outside 0..ldy-1=%lld", col,
                 (long long)ldy - 1);
  STDADK_REQUIRE(grid_sizes_ok(S, nT), STDADK_E_SHAPE, "variogram: S*nT = %lld x %lld rows do not fit 31 bits",
                 (long long)S, (long long)nT);
  STDADK_REQUIRE((S == 0 || nT == 0) || (z && coords), STDADK_E_ARG, "variogram: NULL pointer");
  STDADK_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7) == 0, STDADK_E_ALIGN, "variogram: acc not 8-byte aligned");
  if (int rc = check_workspace("variogram", workspace, workspace_bytes,
                               stdadk_variogram_workspace_bytes(S, nT, n_bins, n_lags),
                               "stdadk_variogram_workspace_bytes"))
    return rc;
  const size_t rows = (size_t)S * (size_t)nT;
  const ByteRange out[2] = {{acc, (size_t)4 * n_lags * n_bins * 4 * sizeof(double)}, {workspace, workspace_bytes}};
  const ByteRange in[4] = {{y_pred, y_pred ? rows * (size_t)ldy * sizeof(float) : 0},
                           {z, rows * sizeof(float)},
                           {split, split ? rows : 0},
                           {coords, (size_t)S * 2 * sizeof(float)}};
  if (int rc = check_no_alias("variogram", out, in, "")) return rc;

  const int G = (int)variogram_blocks(S);
  const int lags_run = S == 0 ? 0 : (int)(n_lags < nT ? n_lags : nT);      // a lag u >= nT has no pair
  hipStream_t st = (hipStream_t)stream;
  if (lags_run > 0) {
    VariogramArgs a;
    a.yp = y_pred; a.z = z; a.coords = coords; a.split = split;
    a.ldy = ldy; a.col = col; a.S = (int)S; a.nT = (int)nT; a.n_bins = n_bins; a.G = G;
    a.part = (double *)workspace;
    for (int b = 0; b <= VG_MAX_BINS; ++b) a.edges2[b] = b <= n_bins ? edges2_host[b] : 0.0;
    if (y_pred)
      STDADK_LAUNCH(variogram_kernel<true>, dim3((unsigned)G, (unsigned)lags_run), dim3(GS_T), 0, st, a);
    else
      STDADK_LAUNCH(variogram_kernel<false>, dim3((unsigned)G, (unsigned)lags_run), dim3(GS_T), 0, st, a);
    STDADK_CHECK_LAUNCH("variogram");
  }
  STDADK_LAUNCH(variogram_finish_kernel, dim3((unsigned)n_bins, (unsigned)n_lags), dim3(GS_T), 0, st,
                (const double *)workspace, G, lags_run, (int)n_bins, (int)n_lags, acc);
  STDADK_CHECK_LAUNCH("variogram_finish");
  return 0;
}
