// Split-conformal calibration on the device (see include/stdadk.h): the conformity scores of one chunk of a site x time
// grid as an ORDERED compaction (stdadk_conformal_scores_f32) and exact order statistics of such scores without a sort
// (stdadk_select_f32).
//
// Scores -- three launches over the chunk's rows r = ti*S + s, cut into RUNS of CS_RUN consecutive rows (a run is the
// "slice" of the compaction: one wave owns it and walks it 64 rows at a time, so its loads are whole 256-byte lines):
//   conformal_count_kernel    the members of every run per segment: popcounts of ballots, one int64 pair per run
//   conformal_scan_kernel     one workgroup: the exclusive scan of the runs' counts (a thread adds a contiguous block
//                             of runs, the 256 block sums are scanned in LDS), started from the device counters; at its
//                             end it advances the counters (saturating at cap) and sets the overflow flags
//   conformal_scatter_kernel  the wave of a run starts from the run's offset; inside 64 rows a member's position is the
//                             popcount of the member ballot below its lane.  A position >= cap is not written.
// The position of an entry is therefore the count of members before it in time-major order: numpy's scores[mask]
// order, with no atomic anywhere, and chunked calls continue where the last one stopped.  A score is one or two float32
// subtractions and a maximum or an absolute value, each rounded once: the bits of numpy float32 arithmetic.
//
// Select -- radix select on order-preserving unsigned keys, SEL_BITS = 8 bits per pass, four passes:
//   select_setup_kernel   reads n, turns a level into a rank, answers "rank beyond n" at once, clears the histograms
//   select_hist_kernel    one sweep over the data per pass for ALL selections: a workgroup keeps ONE set of histograms
//                         (16 selections x 256 bins of uint32 = 16 KiB) in LDS, counts with integer LDS atomics the
//                         keys whose higher digits equal the selection's prefix, then adds its non-zero bins to the
//                         global histograms with integer atomics.  Counts do not depend on the order of arrival.
//   select_pick_kernel    one wave per selection: the bin where the running count crosses the remaining rank becomes the
//                         next digit of the prefix; the histograms are cleared for the next pass
// After the last pass the prefix IS the key of the answer, mapped back to the float: the data is read four times and
// never searched.  In the first pass every key matches, so the selections of one column share the histogram of the
// column's first selection.  8 bits: 4 reads of the data against 3 with 11 bits, but a histogram set of 16 KiB instead
// of 128 KiB, so four workgroups stay resident per CU and the pick is 256 bins per wave.
#include "grid_reduce.h"

namespace stdadk {

constexpr int CS_RUN = 1024;                   // rows per run: 16 steps of one wave
constexpr int CS_WAVES = GS_T / kWave;         // runs per workgroup
constexpr int CS_MAX_C = STDADK_CONFORMAL_MAX_COLS, CS_MAX_G = STDADK_CONFORMAL_MAX_SEGMENTS;
constexpr int SEL_BITS = 8, SEL_BINS = 1 << SEL_BITS, SEL_PASSES = 32 / SEL_BITS;
constexpr int SEL_MAX = STDADK_SELECT_MAX, SEL_T = 256, SEL_U = 4;
constexpr int SEL_MAX_BLOCKS = 1024;           // 4 workgroups per CU on 256 CUs
static_assert(SEL_BITS * SEL_PASSES == 32 && SEL_BINS == 4 * kWave, "select_pick_kernel: four bins per lane");

struct ConformalArgs {
  const float *yp, *z;
  const uint8_t *split;
  int64_t rows;                                // nT * S < 2^31
  int Q, C, G;
  int kind[CS_MAX_C], ca[CS_MAX_C], cb[CS_MAX_C];
  int code[CS_MAX_G];
  int64_t *runs;                               // [nruns][CS_MAX_G]: the counts, then the offsets
};

// member of segment g: a finite value whose code is the segment's
__device__ __forceinline__ bool conformal_member(const ConformalArgs &a, int64_t r, bool live, float &zf, int &code) {
  zf = live ? a.z[r] : __builtin_nanf("");
  code = live && a.split ? (int)a.split[r] : 0;
  return zf - zf == 0.f;
}

__global__ __launch_bounds__(GS_T) void conformal_count_kernel(ConformalArgs a, int64_t nruns) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t run = (int64_t)blockIdx.x * CS_WAVES + wave;
  if (run >= nruns) return;
  int64_t n[CS_MAX_G] = {0, 0};
  for (int i = 0; i < CS_RUN; i += kWave) {
    const int64_t r = run * CS_RUN + i + lane;
    float zf;
    int code;
    const bool ok = conformal_member(a, r, r < a.rows, zf, code);
#pragma unroll
    for (int g = 0; g < CS_MAX_G; ++g) n[g] += __builtin_popcountll(__ballot(ok && g < a.G && code == a.code[g]));
  }
  if (lane < CS_MAX_G) a.runs[run * CS_MAX_G + lane] = lane == 0 ? n[0] : n[1];
}

__global__ __launch_bounds__(GS_T) void conformal_scan_kernel(int64_t *__restrict__ runs, int64_t nruns, int G,
                                                             int64_t cap, int64_t *__restrict__ count,
                                                             int32_t *__restrict__ overflow) {
  __shared__ int64_t part[GS_T];
  const int tid = threadIdx.x;
  const int64_t per = (nruns + GS_T - 1) / GS_T;
  const int64_t lo = tid * per < nruns ? tid * per : nruns, hi = lo + per < nruns ? lo + per : nruns;
  for (int g = 0; g < G; ++g) {
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += runs[i * CS_MAX_G + g];
    __syncthreads();
    part[tid] = s;
    __syncthreads();
    const int64_t start = count[g] > 0 ? count[g] : 0;
    int64_t base = start, total = 0;
    for (int j = 0; j < GS_T; ++j) {           // 256 additions per thread: the launch is one workgroup anyway
      base += j < tid ? part[j] : 0;
      total += part[j];
    }
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t c = runs[i * CS_MAX_G + g];
      runs[i * CS_MAX_G + g] = base;
      base += c;
    }
    __syncthreads();                           // every thread has read count[g]
    if (tid == 0) {
      const bool over = start + total > cap;
      count[g] = over ? cap : start + total;
      if (over) overflow[g] = 1;
    }
  }
}

__global__ __launch_bounds__(GS_T) void conformal_scatter_kernel(ConformalArgs a, int64_t nruns, float *__restrict__ scores,
                                                                int64_t cap) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t run = (int64_t)blockIdx.x * CS_WAVES + wave;
  if (run >= nruns) return;
  int64_t pos[CS_MAX_G];
#pragma unroll
  for (int g = 0; g < CS_MAX_G; ++g) pos[g] = g < a.G ? a.runs[run * CS_MAX_G + g] : 0;
  const uint64_t below = (1ull << lane) - 1ull;
  for (int i = 0; i < CS_RUN; i += kWave) {
    const int64_t r = run * CS_RUN + i + lane;
    if (run * CS_RUN + i >= a.rows) break;     // wave-uniform
    float zf;
    int code;
    const bool ok = conformal_member(a, r, r < a.rows, zf, code);
    bool m[CS_MAX_G];
    uint64_t mb[CS_MAX_G];
#pragma unroll
    for (int g = 0; g < CS_MAX_G; ++g) {
      m[g] = ok && g < a.G && code == a.code[g];
      mb[g] = __ballot(m[g]);
    }
    if ((mb[0] | mb[1]) == 0) continue;        // wave-uniform
    if (m[0] || m[1]) {
      const float *p = a.yp + r * a.Q;
      for (int c = 0; c < a.C; ++c) {
        const float pa = p[a.ca[c]];
        float sc;
        if (a.kind[c] == STDADK_CONFORMAL_CQR) {
          const float pb = p[a.cb[c]];
          const float d0 = pa - zf, d1 = zf - pb;
          sc = d0 > d1 ? d0 : d1;              // finite operands: np.maximum
        } else {
          const float d = zf - pa;
          sc = a.kind[c] == STDADK_CONFORMAL_ABS ? __builtin_fabsf(d) : d;
        }
#pragma unroll
        for (int g = 0; g < CS_MAX_G; ++g) {
          const int64_t at = pos[g] + __builtin_popcountll(mb[g] & below);
          if (m[g] && at >= 0 && at < cap) scores[((int64_t)g * a.C + c) * cap + at] = sc;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < CS_MAX_G; ++g) pos[g] += __builtin_popcountll(mb[g]);
  }
}

// ---- select ----

// the order of the keys as unsigned integers is the order of the floats; -0 counts as +0
__device__ __forceinline__ uint32_t select_key(float f) {
  const uint32_t b = f == 0.f ? 0u : __builtin_bit_cast(uint32_t, f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float select_value(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

struct SelectState {                           // per selection, in the workspace
  uint32_t prefix;                             // the digits found so far, in their place
  int32_t active;                              // 0: answered by the setup (rank beyond n)
  int64_t rank;                                // the rank that is left among the keys that match the prefix
};

struct SelectArgs {
  const float *keys;
  int64_t stride, n_max;
  const int64_t *n_dev;
  int n_sel, n_cols;                           // n_cols: the distinct columns that have a selection
  int col[SEL_MAX];                            // the selection's column
  int lead[SEL_MAX];                           // the first selection of the same column
  int ucol[STDADK_CONFORMAL_MAX_COLS];         // the distinct columns
  int64_t rank[SEL_MAX];                       // >= 0: 0-based, < 0: from beta
  double beta[SEL_MAX];
  SelectState *state;
  uint32_t *hist;                              // [SEL_MAX][SEL_BINS]
  float *value;
  int64_t *rank_used;
};

__device__ __forceinline__ int64_t select_n(const SelectArgs &a) {
  const int64_t n = *a.n_dev;
  return n < 0 ? 0 : (n > a.n_max ? a.n_max : n);
}

__global__ __launch_bounds__(SEL_T) void select_setup_kernel(SelectArgs a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  for (int i = tid; i < SEL_MAX * SEL_BINS; i += SEL_T) a.hist[i] = 0u;
  if (tid >= a.n_sel) return;
  const int64_t n = select_n(a);
  int64_t r = a.rank[tid];
  if (r < 0) {
    const double k = __builtin_ceil((double)(n + 1) * a.beta[tid]);   // the one product, in IEEE double
    r = (k < 1.0 ? (int64_t)1 : (int64_t)k) - 1;
  }
  const bool in = r < n;
  a.state[tid].prefix = 0u;
  a.state[tid].active = in ? 1 : 0;
  a.state[tid].rank = r;
  a.rank_used[tid] = in ? r : -1;
  a.value[tid] = __builtin_inff();             // the answer of a rank beyond n; the last pick overwrites it otherwise
}

__global__ __launch_bounds__(SEL_T) void select_hist_kernel(SelectArgs a, int pass) {
  __shared__ uint32_t h[SEL_MAX][SEL_BINS];
  __shared__ uint32_t s_prefix[SEL_MAX];
  __shared__ int s_on[SEL_MAX];
  const int tid = threadIdx.x;
  const int c = a.ucol[blockIdx.y];
  for (int i = tid; i < SEL_MAX * SEL_BINS; i += SEL_T) (&h[0][0])[i] = 0u;
  if (tid < SEL_MAX) {
    const bool mine = tid < a.n_sel && a.col[tid] == c;
    // first pass: every key matches the empty prefix, the column's first selection counts for all of them
    s_on[tid] = mine && (pass == 0 ? a.lead[tid] == tid : a.state[tid].active != 0);
    s_prefix[tid] = mine ? a.state[tid].prefix : 0u;
  }
  __syncthreads();
  const int64_t n = select_n(a);
  const float *x = a.keys + (int64_t)c * a.stride;
  const int shift = 32 - SEL_BITS * (pass + 1);
  const int64_t step = (int64_t)gridDim.x * SEL_T * SEL_U;
  for (int64_t i0 = (int64_t)blockIdx.x * SEL_T * SEL_U; i0 < n; i0 += step) {
    uint32_t k[SEL_U];
    bool in[SEL_U];
#pragma unroll
    for (int u = 0; u < SEL_U; ++u) {
      const int64_t i = i0 + u * SEL_T + tid;
      in[u] = i < n;
      k[u] = in[u] ? select_key(x[i]) : 0u;
    }
    for (int j = 0; j < a.n_sel; ++j) {
      if (!s_on[j]) continue;                  // workgroup-uniform
      const uint32_t pre = s_prefix[j];
#pragma unroll
      for (int u = 0; u < SEL_U; ++u) {
        // the digits above this pass's: (k ^ pre) >> (shift + SEL_BITS), a shift by 32 in the first pass
        const bool hit = in[u] && (pass == 0 || ((k[u] ^ pre) >> (shift + SEL_BITS)) == 0u);
        const uint32_t d = (k[u] >> shift) & (SEL_BINS - 1);
        // a wave whose hits all fall in one bin (long tie runs, a shared exponent) adds once
        const uint64_t hb = __ballot(hit);
        if (hb == 0) continue;
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)__builtin_ctzll(hb));
        if (__ballot(hit && d == d0) == hb) {
          if ((tid & (kWave - 1)) == (int)__builtin_ctzll(hb)) atomicAdd(&h[j][d0], (uint32_t)__builtin_popcountll(hb));
        } else if (hit) {
          atomicAdd(&h[j][d], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < SEL_MAX * SEL_BINS; i += SEL_T) {
    const uint32_t v = (&h[0][0])[i];
    if (v) atomicAdd(a.hist + i, v);
  }
}

// blockDim = 64 * n_sel: wave j picks the digit of selection j
__global__ __launch_bounds__(kWave * SEL_MAX) void select_pick_kernel(SelectArgs a, int pass) {
  const int lane = threadIdx.x & (kWave - 1), j = threadIdx.x / kWave;
  const int shift = 32 - SEL_BITS * (pass + 1);
  const bool on = a.state[j].active != 0;
  if (on) {
    const uint32_t *hj = a.hist + (size_t)(pass == 0 ? a.lead[j] : j) * SEL_BINS;
    const int64_t r = a.state[j].rank;
    uint32_t b[4];
    int64_t s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      b[q] = hj[lane * 4 + q];
      s += b[q];
    }
    int64_t inc = s;                           // inclusive scan over the lanes
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int64_t up = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += up;
    }
    int64_t e = inc - s;                       // the keys in the bins before this lane's
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (e <= r && r < e + (int64_t)b[q]) {   // exactly one bin of one lane: the counts add up to more than r
        const uint32_t pre = a.state[j].prefix | ((uint32_t)(lane * 4 + q) << shift);
        a.state[j].prefix = pre;
        a.state[j].rank = r - e;
        if (pass == SEL_PASSES - 1) a.value[j] = select_value(pre);
      }
      e += b[q];
    }
  }
  __syncthreads();                             // the selections of a column have read their leader's histogram
  uint32_t *hj = a.hist + (size_t)j * SEL_BINS;
#pragma unroll
  for (int q = 0; q < 4; ++q) hj[lane * 4 + q] = 0u;
}

static inline int64_t conformal_runs(int64_t rows) { return ceil_div(rows > 0 ? rows : 1, CS_RUN); }

}  // namespace stdadk

using namespace stdadk;

extern "C" size_t stdadk_conformal_scores_workspace_bytes(int64_t S, int64_t nT) {
  if (!grid_sizes_ok(S, nT)) return 0;
  return (size_t)conformal_runs(S * nT) * CS_MAX_G * sizeof(int64_t);
}

extern "C" int stdadk_conformal_scores_f32(const float *y_pred, const float *z, const uint8_t *split, int64_t S,
                                           int64_t nT, int32_t Q, const int32_t *cols_host, int32_t C,
                                           const int32_t *codes_host, int32_t G, float *scores, int64_t cap,
                                           int64_t *count, int32_t *overflow, void *workspace, size_t workspace_bytes,
                                           stdadk_stream_t stream) {
  STDADK_REQUIRE(S >= 0 && nT >= 0, STDADK_E_ARG, "conformal_scores: negative size");
  STDADK_REQUIRE(cols_host && codes_host, STDADK_E_ARG, "conformal_scores: NULL descriptor array");
  STDADK_REQUIRE(Q >= 1 && Q <= STDADK_MAX_Q, STDADK_E_ARG, "conformal_scores: Q=%d outside 1..%d", Q, STDADK_MAX_Q);
  STDADK_REQUIRE(C >= 1 && C <= CS_MAX_C, STDADK_E_ARG, "conformal_scores: C=%d score columns outside 1..%d", C, CS_MAX_C);
  STDADK_REQUIRE(G >= 1 && G <= CS_MAX_G, STDADK_E_ARG, "conformal_scores: G=%d segments outside 1..%d", G, CS_MAX_G);
  ConformalArgs a = {};
  for (int c = 0; c < C; ++c) {
    const int kind = cols_host[3 * c], ca = cols_host[3 * c + 1], cb = cols_host[3 * c + 2];
    STDADK_REQUIRE(kind == STDADK_CONFORMAL_RESID || kind == STDADK_CONFORMAL_CQR || kind == STDADK_CONFORMAL_ABS,
                   STDADK_E_ARG, "conformal_scores: column %d has the unknown kind %d", c, kind);
    STDADK_REQUIRE(ca >= 0 && ca < Q && (kind != STDADK_CONFORMAL_CQR || (cb >= 0 && cb < Q)), STDADK_E_ARG,
                   "conformal_scores: column %d names prediction columns (%d, %d) outside 0..%d", c, ca, cb, Q - 1);
    a.kind[c] = kind; a.ca[c] = ca; a.cb[c] = kind == STDADK_CONFORMAL_CQR ? cb : ca;
  }
  for (int g = 0; g < G; ++g) {
    STDADK_REQUIRE(codes_host[g] >= 0 && codes_host[g] <= 255, STDADK_E_ARG,
                   "conformal_scores: split code %d of segment %d outside 0..255", codes_host[g], g);
    a.code[g] = codes_host[g];
  }
  STDADK_REQUIRE(cap >= 0, STDADK_E_ARG, "conformal_scores: negative capacity");
  STDADK_REQUIRE(count && overflow && (scores || cap == 0), STDADK_E_ARG, "conformal_scores: NULL output");
  STDADK_REQUIRE(grid_sizes_ok(S, nT) && cap < (1ll << 31), STDADK_E_SHAPE,
                 "conformal_scores: S*nT = %lld x %lld rows or cap = %lld do not fit 31 bits", (long long)S,
                 (long long)nT, (long long)cap);
  STDADK_REQUIRE((reinterpret_cast<uintptr_t>(count) & 7) == 0 && (reinterpret_cast<uintptr_t>(overflow) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(scores) & 3) == 0,
                 STDADK_E_ALIGN, "conformal_scores: count not 8-byte or scores / overflow not 4-byte aligned");
  if (S == 0 || nT == 0) return 0;
  STDADK_REQUIRE(y_pred && z && workspace, STDADK_E_ARG, "conformal_scores: NULL pointer");
  if (int rc = check_workspace("conformal_scores", workspace, workspace_bytes,
                               stdadk_conformal_scores_workspace_bytes(S, nT), "stdadk_conformal_scores_workspace_bytes"))
    return rc;
  a.yp = y_pred; a.z = z; a.split = split;
  a.rows = S * nT;
  a.Q = Q; a.C = C; a.G = G;
  a.runs = (int64_t *)workspace;
  const int64_t nruns = conformal_runs(a.rows);
  const unsigned nblk = (unsigned)ceil_div(nruns, CS_WAVES);
  hipStream_t st = (hipStream_t)stream;
  STDADK_LAUNCH(conformal_count_kernel, dim3(nblk), dim3(GS_T), 0, st, a, nruns);
  STDADK_CHECK_LAUNCH("conformal_count");
  STDADK_LAUNCH(conformal_scan_kernel, dim3(1), dim3(GS_T), 0, st, a.runs, nruns, (int)G, cap, count, overflow);
  STDADK_CHECK_LAUNCH("conformal_scan");
  STDADK_LAUNCH(conformal_scatter_kernel, dim3(nblk), dim3(GS_T), 0, st, a, nruns, scores, cap);
  STDADK_CHECK_LAUNCH("conformal_scatter");
  return 0;
}

extern "C" size_t stdadk_select_workspace_bytes(int32_t n_sel) {
  if (n_sel < 1 || n_sel > SEL_MAX) return 0;
  return (size_t)SEL_MAX * SEL_BINS * sizeof(uint32_t) + (size_t)SEL_MAX * sizeof(SelectState);
}

extern "C" int stdadk_select_f32(const float *keys, int64_t stride, int32_t C, const int64_t *n_dev, int64_t n_max,
                                 const int32_t *sel_col_host, const int64_t *sel_rank_host,
                                 const double *sel_beta_host, int32_t n_sel, float *value, int64_t *rank_used,
                                 void *workspace, size_t workspace_bytes, stdadk_stream_t stream) {
  STDADK_REQUIRE(n_sel >= 1 && n_sel <= SEL_MAX, STDADK_E_ARG, "select: n_sel=%d outside 1..%d", n_sel, SEL_MAX);
  STDADK_REQUIRE(C >= 1 && C <= CS_MAX_C, STDADK_E_ARG, "select: C=%d columns outside 1..%d", C, CS_MAX_C);
  STDADK_REQUIRE(sel_col_host && sel_rank_host, STDADK_E_ARG, "select: NULL selection array");
  STDADK_REQUIRE(n_max >= 0 && stride >= 0, STDADK_E_ARG, "select: negative size");
  STDADK_REQUIRE(n_dev && value && rank_used && workspace && (keys || n_max == 0), STDADK_E_ARG, "select: NULL pointer");
  SelectArgs a = {};
  for (int j = 0; j < n_sel; ++j) {
    STDADK_REQUIRE(sel_col_host[j] >= 0 && sel_col_host[j] < C, STDADK_E_ARG, "select: selection %d names column %d outside 0..%d",
                   j, sel_col_host[j], C - 1);
    a.col[j] = sel_col_host[j];
    a.rank[j] = sel_rank_host[j];
    a.beta[j] = 0.0;
    if (a.rank[j] < 0) {
      STDADK_REQUIRE(sel_beta_host && sel_beta_host[j] >= 0.0 && sel_beta_host[j] <= 1.0, STDADK_E_ARG,
                     "select: selection %d has no rank and no level in [0, 1]", j);
      a.beta[j] = sel_beta_host[j];
    }
    a.lead[j] = j;
    for (int i = j - 1; i >= 0; --i)
      if (a.col[i] == a.col[j]) a.lead[j] = i;
    if (a.lead[j] == j) a.ucol[a.n_cols++] = a.col[j];
  }
  STDADK_REQUIRE(n_max < (1ll << 31) && stride >= n_max, STDADK_E_SHAPE,
                 "select: n_max=%lld must stay below 2^31 and within the column stride %lld", (long long)n_max,
                 (long long)stride);
  STDADK_REQUIRE((reinterpret_cast<uintptr_t>(n_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(rank_used) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(keys) & 3) == 0 && (reinterpret_cast<uintptr_t>(value) & 3) == 0,
                 STDADK_E_ALIGN, "select: n / rank_used not 8-byte or keys / value not 4-byte aligned");
  if (int rc = check_workspace("select", workspace, workspace_bytes, stdadk_select_workspace_bytes(n_sel),
                               "stdadk_select_workspace_bytes"))
    return rc;
  a.keys = keys; a.stride = stride; a.n_max = n_max; a.n_dev = n_dev; a.n_sel = n_sel;
  a.hist = (uint32_t *)workspace;
  a.state = (SelectState *)(a.hist + (size_t)SEL_MAX * SEL_BINS);
  a.value = value; a.rank_used = rank_used;
  int64_t nblk = ceil_div(n_max > 0 ? n_max : 1, (int64_t)SEL_T * SEL_U);
  if (nblk * a.n_cols > SEL_MAX_BLOCKS) nblk = ceil_div(SEL_MAX_BLOCKS, a.n_cols);
  hipStream_t st = (hipStream_t)stream;
  STDADK_LAUNCH(select_setup_kernel, dim3(1), dim3(SEL_T), 0, st, a);
  STDADK_CHECK_LAUNCH("select_setup");
  for (int pass = 0; pass < SEL_PASSES; ++pass) {
    STDADK_LAUNCH(select_hist_kernel, dim3((unsigned)nblk, (unsigned)a.n_cols), dim3(SEL_T), 0, st, a, pass);
    STDADK_CHECK_LAUNCH("select_hist");
    STDADK_LAUNCH(select_pick_kernel, dim3(1), dim3(kWave * n_sel), 0, st, a, pass);
    STDADK_CHECK_LAUNCH("select_pick");
  }
  return 0;
}
