// Neighbour tables by a cell-binned search (stdadk_knn_cells_f32; see include/stdadk.h): the table of stdadk_knn_f32,
// bit for bit, without meeting every (target, source) pair.  The sites are binned into a uniform G x G grid over the
// box of their finite coordinates; a wave of 64 cell-adjacent targets walks the cells of its own rectangle and then one
// frame of cells per ring, and stops when no lane can still gain a neighbour.
//
// GRID RULE (S alone).  G is the largest g in 1 .. KC_GMAX with KC_OCC g g <= S, and 1 when there is none: about
// KC_OCC sites per cell until the side is clamped.
// CELLS.  x0, x1, y0, y1 are the exact min and max of the coordinates of the sites with BOTH coordinates finite (min
// and max do not depend on the order of a reduction).  A site's column is clamp(floor((x - x0) * (G / (x1 - x0))), 0,
// G - 1) in double, its row likewise from y: MONOTONE in the coordinate, whatever the rounding.  A zero extent (or no
// finite site) gives one column (row).  A site with a non-finite coordinate is LOOSE: cell G G, which every wave walks
// first.  Targets take their cells by the same function of the same four numbers, so a target's column is never left of
// a site with a smaller x; a loose target (NaN or inf) never stops and so meets every source.
// BINNING.  Count, scan and scatter with integer atomics give the sites in cell order (their coordinates as doubles
// next to their index) and the cell starts; the targets are sorted the same way.  The position of a site INSIDE its
// cell, and so the wave a target lands in, may differ from run to run.  The table cannot: a lane's list is the k
// smallest of what it met in the TOTAL order (d2, index), and what it has not met is proved larger.
// EDGES.  Per grid column the exact min and max x of its members, per row of y; from them LX[a] = the largest x of any
// site in a column < a (-inf: none) and RX[b] = the smallest x in a column > b (+inf), LY and RY likewise.
// Launches:
//   knn_cells_init_kernel     the box, the counters and the per-column extremes to their neutral values
//   knn_cells_bounds_kernel   the box: a wave's min / max by shuffles, then one integer atomic min / max per wave
//   knn_cells_count_kernel    a thread per site and per target: its cell, the cell's counter, the column's extremes
//   knn_cells_scan_kernel     three workgroups: the sites' exclusive scan, the targets', and LX / RX / LY / RY
//   knn_cells_scatter_kernel  a thread per site and per target into its cell's run
//   knn_cells_search_kernel<KT>  one wave per 64 sorted targets and slice.  The cells of a grid row between two columns
//                        are ONE run of the sorted sites: the wave stages 64 of them in LDS (coalesced; the slice's
//                        flag gathered by index) and every lane reads the same staged source, as in knn_search_kernel;
//                        a non-source is skipped by the whole wave.  Sources arrive in no index order, so every
//                        insertion is the total one.  The rows come back in the caller's order: a lane writes row j.
// THE PROOF OBLIGATION.  A source is skipped only when a value has been computed that is <= its d2 by monotonicity of
// the same rounded operations, and that value is STRICTLY greater than the lane's current k-th key.  After the
// rectangle [a0, a1] x [r0, r1] every site not met lies in a column < a0, a column > a1, a row < r0 or a row > r1.
// For the first: its x <= LX[a0] <= qx (cells are monotone), so qx - x >= qx - LX[a0] >= 0 exactly, the rounded
// differences keep that order, so do their rounded squares, and d2 = fl(dx dx + dy dy) >= fl(dx dx): the squared gap,
// ONE difference and ONE product each rounded once, is never above d2.  The other three sides alike; the bound is the
// least of the four, and a gap that is not positive gives 0.  Equality must visit (an equal distance at a lower index
// belongs in the row), so a lane is done only when its list is full and `bound > worst` is TRUE: a NaN on either side
// -- an empty slot's key read as a double is one -- prunes nothing, and neither does a bound of +inf against a k-th
// distance of +inf.  The wave goes on while a ballot finds a lane that is not done, and stops at the latest when the
// rectangle is the grid: at most G rings.  No nominal cell edge x0 + i h is ever compared against, and no operation of
// d2 or of the bound is contracted.
#include "knn_common.h"

namespace stdadk {

constexpr int KC_OCC = 4;                      // sites per cell the grid rule aims at
constexpr int KC_GMAX = 1024;                  // grid side at the most
constexpr int KC_T = 256;                      // threads per workgroup of the binning kernels
constexpr int KC_SCAN_T = 1024;                // threads of a scan workgroup
constexpr int KC_MT = kWave;                   // targets per search workgroup: ONE wave, a lane each

static inline int64_t kc_grid_side(int64_t S) {
  int64_t g = 1;
  while (g < KC_GMAX && (g + 1) * (g + 1) * KC_OCC <= S) ++g;
  return g;
}

// the workspace: every array's offset in bytes, each a multiple of 8
struct KcPlan {
  int64_t G, cells;                            // cells = G G + 1, the last one the loose bucket
  size_t box, edge, band, s_cur, s_start, t_cur, s_cell, t_cell, s_idx, t_ord, s_x, s_y, bytes;
};
static inline KcPlan kc_plan(int64_t M, int64_t S) {
  KcPlan p;
  p.G = kc_grid_side(S);
  p.cells = p.G * p.G + 1;
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t here = at;
    at += align_up(bytes, 8);
    return here;
  };
  p.box = take(4 * sizeof(unsigned));
  p.edge = take(4 * (size_t)p.G * sizeof(double));
  p.band = take(4 * (size_t)p.G * sizeof(unsigned));
  p.s_cur = take((size_t)p.cells * sizeof(unsigned));
  p.s_start = take((size_t)(p.cells + 1) * sizeof(unsigned));
  p.t_cur = take((size_t)p.cells * sizeof(unsigned));
  p.s_cell = take((size_t)S * sizeof(int));
  p.t_cell = take((size_t)M * sizeof(int));
  p.s_idx = take((size_t)S * sizeof(int));
  p.t_ord = take((size_t)M * sizeof(int));
  p.s_x = take((size_t)S * sizeof(double));
  p.s_y = take((size_t)S * sizeof(double));
  p.bytes = at;
  return p;
}

struct KcArgs {
  const float *q, *coords;
  const uint8_t *src;
  int M, S, G, cells, tiles, k, exclude_self;
  unsigned *box;                               // min x, max x, min y, max y as ordered integers
  double *edge;                                // LX[G], RX[G], LY[G], RY[G]
  unsigned *band;                              // per column min x, max x; per row min y, max y (ordered integers)
  unsigned *s_cur, *s_start, *t_cur;           // counters, then cursors; the sites' cell starts
  int *s_cell, *t_cell, *s_idx, *t_ord;
  double *s_x, *s_y;
  int *nbr_idx;
  double *nbr_d2;
};

// a float as an unsigned integer of the same order (finite values and the infinities; -0 below +0)
__device__ __forceinline__ unsigned kc_enc(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ double kc_dec(unsigned e) {
  return (double)__uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}
__device__ __forceinline__ bool kc_finite(float x, float y) { return isfinite(x) && isfinite(y); }

// the box as the cell function uses it: origin and cells per unit on each axis (0: one column / row)
struct KcFrame {
  double x0, y0, ix, iy;
};
__device__ __forceinline__ KcFrame kc_frame(const unsigned *box, int G) {
#pragma clang fp contract(off)
  KcFrame f = {0.0, 0.0, 0.0, 0.0};
  if (box[0] <= box[1]) {                      // a finite site exists
    f.x0 = kc_dec(box[0]);
    f.y0 = kc_dec(box[2]);
    const double ex = kc_dec(box[1]) - f.x0, ey = kc_dec(box[3]) - f.y0;
    f.ix = ex > 0.0 ? (double)G / ex : 0.0;
    f.iy = ey > 0.0 ? (double)G / ey : 0.0;
  }
  return f;
}
__device__ __forceinline__ int kc_axis(double v, double v0, double inv, int G) {
#pragma clang fp contract(off)
  const double t = floor((v - v0) * inv);
  return t >= (double)(G - 1) ? G - 1 : t > 0.0 ? (int)t : 0;
}
__device__ __forceinline__ int kc_cell(const KcFrame &f, float x, float y, int G) {
  if (!kc_finite(x, y)) return G * G;
  return kc_axis((double)y, f.y0, f.iy, G) * G + kc_axis((double)x, f.x0, f.ix, G);
}

__global__ __launch_bounds__(KC_T) void knn_cells_init_kernel(KcArgs a) {
  const long long t = (long long)blockIdx.x * KC_T + threadIdx.x;
  if (t < 4) a.box[t] = (t & 1) ? 0u : 0xffffffffu;
  if (t < 4 * (long long)a.G) a.band[t] = ((t / a.G) & 1) ? 0u : 0xffffffffu;
  if (t < a.cells) {
    a.s_cur[t] = 0;
    a.t_cur[t] = 0;
  }
}

__device__ __forceinline__ unsigned kc_wave_min(unsigned v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const unsigned u = (unsigned)__shfl_xor((int)v, o);
    v = u < v ? u : v;
  }
  return v;
}
__device__ __forceinline__ unsigned kc_wave_max(unsigned v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const unsigned u = (unsigned)__shfl_xor((int)v, o);
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(KC_T) void knn_cells_bounds_kernel(KcArgs a) {
  const long long i = (long long)blockIdx.x * KC_T + threadIdx.x;
  unsigned lo_x = 0xffffffffu, hi_x = 0u, lo_y = 0xffffffffu, hi_y = 0u;
  if (i < a.S) {
    const float x = a.coords[2 * (size_t)i], y = a.coords[2 * (size_t)i + 1];
    if (kc_finite(x, y)) {
      lo_x = hi_x = kc_enc(x);
      lo_y = hi_y = kc_enc(y);
    }
  }
  lo_x = kc_wave_min(lo_x);
  hi_x = kc_wave_max(hi_x);
  lo_y = kc_wave_min(lo_y);
  hi_y = kc_wave_max(hi_y);
  if (threadIdx.x % kWave == 0 && lo_x <= hi_x) {
    atomicMin(&a.box[0], lo_x);
    atomicMax(&a.box[1], hi_x);
    atomicMin(&a.box[2], lo_y);
    atomicMax(&a.box[3], hi_y);
  }
}

__global__ __launch_bounds__(KC_T) void knn_cells_count_kernel(KcArgs a) {
  const long long t = (long long)blockIdx.x * KC_T + threadIdx.x;
  if (t >= (long long)a.S + a.M) return;
  const KcFrame f = kc_frame(a.box, a.G);
  const int G = a.G;
  if (t < a.S) {
    const float x = a.coords[2 * (size_t)t], y = a.coords[2 * (size_t)t + 1];
    const int cell = kc_cell(f, x, y, G);
    a.s_cell[t] = cell;
    atomicAdd(&a.s_cur[cell], 1u);
    if (cell < G * G) {
      const int cx = cell % G, cy = cell / G;
      atomicMin(&a.band[cx], kc_enc(x));
      atomicMax(&a.band[G + cx], kc_enc(x));
      atomicMin(&a.band[2 * G + cy], kc_enc(y));
      atomicMax(&a.band[3 * G + cy], kc_enc(y));
    }
  } else {
    const size_t j = (size_t)(t - a.S);
    const int cell = kc_cell(f, a.q[2 * j], a.q[2 * j + 1], G);
    a.t_cell[j] = cell;
    atomicAdd(&a.t_cur[cell], 1u);
  }
}

// Workgroup 0: the sites' counters into their exclusive scan (s_start, with the total behind the last cell) and into
// cursors; workgroup 1: the targets' counters into cursors; workgroup 2: the four edge arrays, a thread each.
__global__ __launch_bounds__(KC_SCAN_T) void knn_cells_scan_kernel(KcArgs a) {
  __shared__ unsigned tot[KC_SCAN_T];
  const int tid = threadIdx.x;
  if (blockIdx.x == 2) {
    if (tid >= 4) return;
    const int G = a.G;
    const unsigned *lo = a.band + (tid < 2 ? 0 : 2 * G), *hi = lo + G;
    double *out = a.edge + (size_t)tid * G;
    if (tid % 2 == 0) {                        // LX, LY: the largest coordinate in a column (row) below
      double run = -__builtin_inf();
      for (int c = 0; c < G; ++c) {
        out[c] = run;
        if (lo[c] <= hi[c]) run = fmax(run, kc_dec(hi[c]));
      }
    } else {                                   // RX, RY: the smallest coordinate in a column (row) above
      double run = __builtin_inf();
      for (int c = G - 1; c >= 0; --c) {
        out[c] = run;
        if (lo[c] <= hi[c]) run = fmin(run, kc_dec(lo[c]));
      }
    }
    return;
  }
  unsigned *cur = blockIdx.x == 0 ? a.s_cur : a.t_cur;
  const int n = a.cells, per = (n + KC_SCAN_T - 1) / KC_SCAN_T;
  const int b = tid * per < n ? tid * per : n, e = b + per < n ? b + per : n;
  unsigned sum = 0;
  for (int c = b; c < e; ++c) sum += cur[c];
  tot[tid] = sum;
  __syncthreads();
  for (int o = 1; o < KC_SCAN_T; o <<= 1) {    // inclusive scan of the threads' sums
    const unsigned add = tid >= o ? tot[tid - o] : 0u;
    __syncthreads();
    tot[tid] += add;
    __syncthreads();
  }
  unsigned run = tot[tid] - sum;
  for (int c = b; c < e; ++c) {
    const unsigned cnt = cur[c];
    cur[c] = run;
    if (blockIdx.x == 0) a.s_start[c] = run;
    run += cnt;
  }
  if (blockIdx.x == 0 && tid == KC_SCAN_T - 1) a.s_start[n] = tot[tid];
}

__global__ __launch_bounds__(KC_T) void knn_cells_scatter_kernel(KcArgs a) {
  const long long t = (long long)blockIdx.x * KC_T + threadIdx.x;
  if (t >= (long long)a.S + a.M) return;
  if (t < a.S) {
    const unsigned at = atomicAdd(&a.s_cur[a.s_cell[t]], 1u);
    a.s_idx[at] = (int)t;
    a.s_x[at] = (double)a.coords[2 * (size_t)t];
    a.s_y[at] = (double)a.coords[2 * (size_t)t + 1];
  } else {
    const long long j = t - a.S;
    a.t_ord[atomicAdd(&a.t_cur[a.t_cell[j]], 1u)] = (int)j;
  }
}

// the squared gap to the nearest coordinate not yet met on one side: one difference (the caller's), one product
__device__ __forceinline__ double kc_gap2(double gap) {
#pragma clang fp contract(off)
  return gap > 0.0 ? gap * gap : 0.0;
}

template <int KT>
__global__ __launch_bounds__(KC_MT) void knn_cells_search_kernel(KcArgs a) {
#pragma clang fp contract(off)
  __shared__ double sx[KC_MT], sy[KC_MT];
  __shared__ int si[KC_MT];
  const int lane = threadIdx.x, G = a.G;
  const int m = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const long long p = (long long)tile * KC_MT + lane;
  const bool mine = p < a.M;
  const int j = a.t_ord[mine ? p : (long long)tile * KC_MT];      // (a lane without a target stands on the tile's first)
  const int cell = a.t_cell[j];
  const bool loose = cell == G * G;
  const double qx = (double)a.q[2 * (size_t)j], qy = (double)a.q[2 * (size_t)j + 1];
  const int cx = loose ? 0 : cell % G, cy = loose ? 0 : cell / G;
  const int self = a.exclude_self ? j : -1;
  const uint8_t *flags = a.src ? a.src + (size_t)m * a.S : nullptr;
  u64 key[KT];
  int ix[KT];
#pragma unroll
  for (int e = 0; e < KT; ++e) {
    key[e] = KN_EMPTY;
    ix[e] = KN_NONE;
  }
  // the sorted sites [b, e), wave-uniform: 64 staged at a time, every lane against every staged source
  auto walk = [&](unsigned b, unsigned e) __attribute__((always_inline)) {
    for (unsigned s0 = b; s0 < e; s0 += KC_MT) {
      const int nv = (int)(e - s0 < (unsigned)KC_MT ? e - s0 : (unsigned)KC_MT);
      __syncthreads();
      if (lane < nv) {
        const int i = a.s_idx[s0 + lane];
        sx[lane] = a.s_x[s0 + lane];
        sy[lane] = a.s_y[s0 + lane];
        si[lane] = (flags ? flags[i] != 0 : true) ? i : -1;
      }
      __syncthreads();
      for (int v = 0; v < nv; ++v) {
        const int i = si[v];
        if (i < 0) continue;                   // (the same for every lane)
        const u64 c = (u64)__double_as_longlong(sq_dist_f64(qx, qy, sx[v], sy[v]));
        if ((c < key[KT - 1] || (c == key[KT - 1] && i < ix[KT - 1])) && i != self) knn_insert<KT, true>(key, ix, c, i);
      }
    }
  };
  int a0 = __builtin_amdgcn_readfirstlane((int)kc_wave_min((unsigned)cx));
  int a1 = __builtin_amdgcn_readfirstlane((int)kc_wave_max((unsigned)cx));
  int r0 = __builtin_amdgcn_readfirstlane((int)kc_wave_min((unsigned)cy));
  int r1 = __builtin_amdgcn_readfirstlane((int)kc_wave_max((unsigned)cy));
  int pa0 = 0, pa1 = -1, pr0 = 0, pr1 = -1;    // the rectangle already met: none
  const double *LX = a.edge, *RX = a.edge + G, *LY = a.edge + 2 * G, *RY = a.edge + 3 * G;
  walk(a.s_start[(size_t)G * G], a.s_start[(size_t)G * G + 1]);      // the loose sites
  for (;;) {
    // what [a0, a1] x [r0, r1] adds to the rectangle already met: whole rows above and below it, and in its own rows
    // the columns left and right of it.  The cells of a grid row between two columns are ONE run of the sorted sites.
    for (int r = r0; r <= r1; ++r) {
      const bool inner = r >= pr0 && r <= pr1;
      for (int side = 0; side < 2; ++side) {
        const int c0 = side == 0 ? a0 : pa1 + 1, c1 = side == 0 ? (inner ? pa0 - 1 : a1) : (inner ? a1 : -1);
        if (c0 <= c1) walk(a.s_start[(size_t)r * G + c0], a.s_start[(size_t)r * G + c1 + 1]);
      }
    }
    if (a0 == 0 && a1 == G - 1 && r0 == 0 && r1 == G - 1) break;      // the rectangle is the grid
    u64 kth = key[0];
#pragma unroll
    for (int e = 1; e < KT; ++e) kth = e < a.k ? key[e] : kth;
    const double worst = __longlong_as_double((long long)kth);       // NaN while the list is short
    const double bx = fmin(kc_gap2(qx - LX[a0]), kc_gap2(RX[a1] - qx));
    const double by = fmin(kc_gap2(qy - LY[r0]), kc_gap2(RY[r1] - qy));
    const bool done = !mine || (!loose && fmin(bx, by) > worst);
    if (__ballot(!done) == 0) break;
    pa0 = a0; pa1 = a1; pr0 = r0; pr1 = r1;
    a0 = a0 > 0 ? a0 - 1 : 0;
    a1 = a1 < G - 1 ? a1 + 1 : G - 1;
    r0 = r0 > 0 ? r0 - 1 : 0;
    r1 = r1 < G - 1 ? r1 + 1 : G - 1;
  }
  if (!mine) return;
  const size_t row = ((size_t)m * a.M + (size_t)j) * a.k;
#pragma unroll
  for (int e = 0; e < KT; ++e)
    if (e < a.k) knn_store_slot(a.nbr_idx, a.nbr_d2, row + e, key[e], ix[e]);
}

}  // namespace stdadk

using namespace stdadk;

extern "C" size_t stdadk_knn_cells_workspace_bytes(int64_t M, int64_t S, int64_t nM, int32_t k) {
  if (!knn_sizes_ok(M, S, nM, k)) return 0;
  return kc_plan(M, S).bytes;                  // (never 0: the box alone is 16 bytes)
}

extern "C" int stdadk_knn_cells_f32(const float *q, int64_t M, const float *coords, int64_t S, const uint8_t *src,
                                    int64_t nM, int32_t k, int32_t exclude_self, int32_t *nbr_idx, double *nbr_d2,
                                    void *workspace, size_t workspace_bytes, stdadk_stream_t stream) {
  if (int rc = knn_check_call("knn_cells", q, M, coords, S, src, nM, k, exclude_self, nbr_idx, nbr_d2, workspace,
                              workspace_bytes, stdadk_knn_cells_workspace_bytes(M, S, nM, k),
                              "stdadk_knn_cells_workspace_bytes"))
    return rc;
  if (M == 0 || nM == 0) return 0;

  const KcPlan p = kc_plan(M, S);
  char *ws = (char *)workspace;
  KcArgs a;
  a.q = q; a.coords = coords; a.src = src;
  a.M = (int)M; a.S = (int)S; a.G = (int)p.G; a.cells = (int)p.cells; a.tiles = (int)ceil_div(M, KC_MT); a.k = k;
  a.exclude_self = exclude_self;
  a.box = (unsigned *)(ws + p.box); a.edge = (double *)(ws + p.edge); a.band = (unsigned *)(ws + p.band);
  a.s_cur = (unsigned *)(ws + p.s_cur); a.s_start = (unsigned *)(ws + p.s_start); a.t_cur = (unsigned *)(ws + p.t_cur);
  a.s_cell = (int *)(ws + p.s_cell); a.t_cell = (int *)(ws + p.t_cell); a.s_idx = (int *)(ws + p.s_idx);
  a.t_ord = (int *)(ws + p.t_ord); a.s_x = (double *)(ws + p.s_x); a.s_y = (double *)(ws + p.s_y);
  a.nbr_idx = nbr_idx; a.nbr_d2 = nbr_d2;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_init = p.cells > 4 * p.G ? p.cells : 4 * p.G;      // (at least 4: the box)
  const dim3 init((unsigned)ceil_div(n_init, KC_T)), sites((unsigned)ceil_div(S, KC_T)),
      both((unsigned)ceil_div(S + M, KC_T)), search((unsigned)(a.tiles * nM));
  STDADK_LAUNCH(knn_cells_init_kernel, init, dim3(KC_T), 0, st, a);
  STDADK_CHECK_LAUNCH("knn_cells_init");
  if (S > 0) {
    STDADK_LAUNCH(knn_cells_bounds_kernel, sites, dim3(KC_T), 0, st, a);
    STDADK_CHECK_LAUNCH("knn_cells_bounds");
  }
  STDADK_LAUNCH(knn_cells_count_kernel, both, dim3(KC_T), 0, st, a);
  STDADK_CHECK_LAUNCH("knn_cells_count");
  STDADK_LAUNCH(knn_cells_scan_kernel, dim3(3), dim3(KC_SCAN_T), 0, st, a);
  STDADK_CHECK_LAUNCH("knn_cells_scan");
  STDADK_LAUNCH(knn_cells_scatter_kernel, both, dim3(KC_T), 0, st, a);
  STDADK_CHECK_LAUNCH("knn_cells_scatter");
#define STDADK_KC_FOR_K(KT)                                                                      \
  do {                                                                                           \
    STDADK_LAUNCH(knn_cells_search_kernel<KT>, search, dim3(KC_MT), 0, st, a);                   \
    STDADK_CHECK_LAUNCH("knn_cells_search");                                                     \
  } while (0)
  if (k == 1)
    STDADK_KC_FOR_K(1);
  else if (k == 2)
    STDADK_KC_FOR_K(2);
  else if (k <= 4)
    STDADK_KC_FOR_K(4);
  else if (k <= 8)
    STDADK_KC_FOR_K(8);
  else
    STDADK_KC_FOR_K(16);
#undef STDADK_KC_FOR_K
  return 0;
}
