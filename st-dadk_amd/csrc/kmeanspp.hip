// Greedy k-means++ seeding in two dimensions, entirely in float64 (stdadk_kmeanspp_f64, contract in include/stdadk.h):
// the data-dependent part of sklearn's _kmeans_plusplus with unit sample weights.  The random stream does not depend on
// the data, so the host draws it in advance -- one first row per run, L uniforms per further centre -- and the kernel
// does the distances, the prefix sums, the picks and the arg-min.
//
// One workgroup of KPP_T threads per run: step c needs step c - 1's result, and the runs are independent.  No atomics,
// nothing waits on another workgroup.  Thread t owns the contiguous rows [t R, (t + 1) R) and keeps their coordinates
// and closest distances d in registers (RegRows<R>, n <= KPP_T * KPP_MAX_R = 10 240); beyond that d lives in the
// workspace and the coordinates are read from X again (MemRows: correct for any n, not meant to be fast).
//
// One step, three barriers:
//   B  every thread: for each candidate j its chunk's sum_r min(d_r, |x_r - cand_j|^2), rows in order from 0.0, into
//      part[j][t].  For the chosen candidate this IS the chunk sum of the updated d, so no sum is formed twice.
//   C  wave j scans part[j]: lanes g < 32 each run through the 32 chunk sums of group g in order (exclusive running sum
//      W_t written in place, the group's total kept), then the 32 group totals are added in order through __shfl (every
//      lane the same chain): Gx_g exclusive, the grand total = pot_j.  The L scans run side by side on L waves.
//   D  every thread: arg-min over pot_j (lowest j on ties), d_r = min(d_r, |x_r - cand_best|^2), and with W_t, Gx_g of
//      the chosen candidate's scan the prefix sum of row r of thread t is
//          P = Gx_g + (W_t + l_r),   l_r = d_0 + ... + d_r of the chunk, in order
//      -- non-decreasing in the row index by construction (W_t + l_last is bitwise W_t+1, Gx_g + total_g is bitwise
//      Gx_g+1, and adding a non-negative term never lowers a rounded sum), and P of the last row is bitwise pot.  The
//      thread whose interval (P before its first row, P of its last row] holds r_j = u_j pot walks its chunk to the
//      crossing row and publishes the candidate (row, coordinates) for the next step.  Exactly one thread owns each r_j;
//      a slot nobody owns (only possible with u >= 1) keeps its preset, row n - 1.
// The candidate slots are double-buffered by the step's parity; the next step's uniforms are loaded in B and reach LDS in C.
// The first centre is step 0 with one candidate, `first`, and d = +inf.  The distance is sq_dist_f64 of f64_block.h.
// Fixed orders throughout: the same call gives the same bits, and two candidates with the same coordinates get the same
// pot_j.  pot == 0: every r_j is 0, thread 0 owns it and row 0 crosses.
#include "f64_block.h"

namespace stdadk {

constexpr int KPP_T = 1024;                // threads per workgroup
constexpr int KPP_G = 32;                  // chunk sums per scan group, and scan groups
constexpr int KPP_STRIDE = KPP_T + KPP_T / KPP_G;     // part[j][t + t / 32]: lane g's column 33 g + q is conflict-free
constexpr int KPP_MAX_L = 16;              // candidates per step, at most (one scanning wave each)
constexpr int KPP_MAX_R = 10;              // rows per thread held in registers, at most
constexpr int KPP_MAX_RUNS = 64;
constexpr int KPP_MAX_K = 65536;
static_assert(KPP_G * KPP_G == KPP_T && KPP_G <= kWave && KPP_MAX_L <= KPP_T / kWave, "one wave scans one candidate");

// rows [tid R, (tid + 1) R) in registers; rows past n are (0, 0) with d = 0 and add 0.0 to every sum
template <int R>
struct RegRows {
  double x[R], y[R], d[R];
  int64_t row0;
  __device__ __forceinline__ void init(const double *__restrict__ X, int64_t n, double *, int tid) {
    row0 = (int64_t)tid * R;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = row0 + r;
      const bool live = i < n;
      x[r] = live ? X[2 * i] : 0.0;
      y[r] = live ? X[2 * i + 1] : 0.0;
      d[r] = live ? __builtin_inf() : 0.0;
    }
  }
  template <class F>
  __device__ __forceinline__ void each(F f) {
#pragma unroll
    for (int r = 0; r < R; ++r) f(r, x[r], y[r], d[r]);
  }
};

// rows [tid rows, (tid + 1) rows) clipped to n, d in the workspace
struct MemRows {
  const double *X;
  double *d;
  int64_t row0, row1;
  __device__ __forceinline__ void init(const double *__restrict__ X_, int64_t n, double *d_, int tid) {
    const int64_t rows = (n + KPP_T - 1) / KPP_T;
    X = X_;
    d = d_;
    row0 = (int64_t)tid * rows < n ? (int64_t)tid * rows : n;
    row1 = row0 + rows < n ? row0 + rows : n;
    for (int64_t i = row0; i < row1; ++i) d[i] = __builtin_inf();
  }
  template <class F>
  __device__ __forceinline__ void each(F f) {
    for (int64_t i = row0; i < row1; ++i) {
      const double old = d[i];
      double v = old;
      f(i - row0, X[2 * i], X[2 * i + 1], v);
      if (v != old) d[i] = v;
    }
  }
};

template <class Rows>
__global__ __launch_bounds__(KPP_T) void kmeanspp_kernel(const double *__restrict__ X, int64_t n, int k, int L,
                                                         const int32_t *__restrict__ first,
                                                         const double *__restrict__ u, int32_t *__restrict__ idx_out,
                                                         double *__restrict__ pot_out, double *__restrict__ dws) {
  extern __shared__ double part[];           // [L][KPP_STRIDE]
  __shared__ double gxs[KPP_MAX_L][KPP_G], potj[KPP_MAX_L], us[KPP_MAX_L];
  __shared__ double cand_x[2][KPP_MAX_L], cand_y[2][KPP_MAX_L];
  __shared__ int cand_i[2][KPP_MAX_L];
  const int tid = threadIdx.x, run = blockIdx.x, wave = tid >> 6, lane = tid & 63;
  const int slot = tid + tid / KPP_G;
  Rows rows;
  rows.init(X, n, dws + (size_t)run * n, tid);
  const double xl = X[2 * (n - 1)], yl = X[2 * (n - 1) + 1];
  const double *ur = u + (size_t)run * (k - 1) * L;         // k == 1: never read
  if (tid == 0) {
    int64_t f = first[run];
    f = f < 0 ? 0 : (f >= n ? n - 1 : f);
    cand_i[0][0] = (int)f;
    cand_x[0][0] = X[2 * f];
    cand_y[0][0] = X[2 * f + 1];
  }
  __syncthreads();
  for (int c = 0; c < k; ++c) {
    const int Lc = c == 0 ? 1 : L, cur = c & 1, nxt = cur ^ 1;
    double unext = 0.0;                      // u[c][tid], the thresholds' uniforms of step c + 1
    if (tid < L && c + 1 < k) unext = ur[(size_t)c * L + tid];
    // B: the chunk's share of every candidate's potential
#pragma nounroll
    for (int j = 0; j < Lc; ++j) {
      const double cx = cand_x[cur][j], cy = cand_y[cur][j];
      double acc = 0.0;
      rows.each([&](int64_t, double x, double y, double &d) {
        const double q = sq_dist_f64(x, y, cx, cy);
        acc += q < d ? q : d;
      });
      part[j * KPP_STRIDE + slot] = acc;
    }
    __syncthreads();
    // C: wave j scans candidate j
    if (wave < Lc) {
      double *p = part + wave * KPP_STRIDE;
      double tot = 0.0;
      if (lane < KPP_G) {
        double *b = p + lane * (KPP_G + 1);
#pragma unroll 4
        for (int q = 0; q < KPP_G; ++q) {
          const double v = b[q];
          b[q] = tot;
          tot += v;
        }
      }
      double gx = 0.0, acc = 0.0;
#pragma unroll 4
      for (int q = 0; q < KPP_G; ++q) {
        const double tq = __shfl(tot, q, kWave);
        if (lane == q) gx = acc;
        acc += tq;
      }
      if (lane < KPP_G) gxs[wave][lane] = gx;
      if (lane == 0) potj[wave] = acc;
    }
    if (tid < L) {
      us[tid] = unext;
      cand_i[nxt][tid] = (int)(n - 1);
      cand_x[nxt][tid] = xl;
      cand_y[nxt][tid] = yl;
    }
    __syncthreads();
    // D: the choice, the update, the next candidates
    int best = 0;
    double pot = potj[0];
    for (int j = 1; j < Lc; ++j) {
      const double pj = potj[j];
      if (pj < pot) {
        pot = pj;
        best = j;
      }
    }
    if (tid == 0) idx_out[(size_t)run * k + c] = cand_i[cur][best];
    if (c + 1 == k) {
      if (tid == 0) pot_out[run] = pot;
      break;
    }
    const double bx = cand_x[cur][best], by = cand_y[cur][best];
    const double W = part[best * KPP_STRIDE + slot], Gx = gxs[best][tid / KPP_G];
    double l = 0.0;
    rows.each([&](int64_t, double x, double y, double &d) {
      const double q = sq_dist_f64(x, y, bx, by);
      if (q < d) d = q;
      l += d;
    });
    const double before = Gx + W, last = Gx + (W + l);
#pragma nounroll
    for (int j = 0; j < L; ++j) {
      const double thr = us[j] * pot;
      if ((tid == 0 || before < thr) && thr <= last) {
        double l2 = 0.0;
        bool found = false;
        rows.each([&](int64_t r, double x, double y, double &d) {
          l2 += d;
          if (!found && Gx + (W + l2) >= thr) {
            found = true;
            cand_i[nxt][j] = (int)(rows.row0 + r);
            cand_x[nxt][j] = x;
            cand_y[nxt][j] = y;
          }
        });
      }
    }
    __syncthreads();
  }
}

static inline bool kpp_sizes_ok(int64_t n, int32_t k, int32_t runs) {
  return n >= 1 && n < (1ll << 31) && k >= 1 && k <= KPP_MAX_K && k <= n && runs >= 1 && runs <= KPP_MAX_RUNS;
}
static inline bool kpp_in_registers(int64_t n) { return n <= (int64_t)KPP_T * KPP_MAX_R; }

template <class Rows>
static int kpp_launch(const double *X, int64_t n, int32_t k, int32_t runs, int32_t L, const int32_t *first,
                      const double *u, int32_t *idx_out, double *pot_out, double *dws, hipStream_t st) {
  auto kern = kmeanspp_kernel<Rows>;
  // once per kernel: the cap for the largest L, so that no later call (a captured one included) has to raise it
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void *>(kern), KPP_MAX_L * KPP_STRIDE * (int)sizeof(double));
    if (e != hipSuccess) { set_error("kmeanspp: LDS attribute: %s", hipGetErrorString(e)); return (int)e; }
    attr_set = true;
  }
  const size_t lds = (size_t)L * KPP_STRIDE * sizeof(double);
  STDADK_LAUNCH_NAMED("kmeanspp_kernel", kern, dim3((unsigned)runs), dim3(KPP_T), lds, st, X, n, (int)k, (int)L, first, u,
                      idx_out, pot_out, dws);
  STDADK_CHECK_LAUNCH("kmeanspp");
  return 0;
}

}  // namespace stdadk

using namespace stdadk;

// workspace: d [runs][n] beyond the register path; 8 bytes (unused) otherwise, so that 0 keeps meaning bad sizes
extern "C" size_t stdadk_kmeanspp_workspace_bytes(int64_t n, int32_t k, int32_t runs) {
  if (!kpp_sizes_ok(n, k, runs)) return 0;
  return kpp_in_registers(n) ? sizeof(double) : (size_t)runs * (size_t)n * sizeof(double);
}

extern "C" int stdadk_kmeanspp_f64(const double *X, int64_t n, int32_t k, int32_t runs, int32_t L, const int32_t *first,
                                   const double *u, int32_t *idx_out, double *pot_out, void *workspace,
                                   size_t workspace_bytes, stdadk_stream_t stream) {
  STDADK_REQUIRE(n >= 1 && n < (1ll << 31), STDADK_E_ARG, "kmeanspp: n=%lld outside 1..2^31-1", (long long)n);
  STDADK_REQUIRE(k >= 1 && k <= KPP_MAX_K && k <= n, STDADK_E_ARG, "kmeanspp: k=%d outside 1..min(n, %d), n=%lld", k,
                 KPP_MAX_K, (long long)n);
  STDADK_REQUIRE(runs >= 1 && runs <= KPP_MAX_RUNS, STDADK_E_ARG, "kmeanspp: runs=%d outside 1..%d", runs, KPP_MAX_RUNS);
  STDADK_REQUIRE(L >= 1 && L <= KPP_MAX_L, STDADK_E_ARG, "kmeanspp: L=%d outside 1..%d", L, KPP_MAX_L);
  STDADK_REQUIRE(X && first && idx_out && pot_out && workspace && (u || k == 1), STDADK_E_ARG, "kmeanspp: NULL pointer");
  const size_t need = stdadk_kmeanspp_workspace_bytes(n, k, runs);
  STDADK_REQUIRE(workspace_bytes >= need, STDADK_E_WORKSPACE,
                 "kmeanspp: workspace %zu < %zu bytes (stdadk_kmeanspp_workspace_bytes)", workspace_bytes, need);
  const auto misaligned = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  STDADK_REQUIRE(!misaligned(X, 8) && !misaligned(u, 8) && !misaligned(pot_out, 8) && !misaligned(workspace, 8),
                 STDADK_E_ALIGN, "kmeanspp: X, u, pot_out and the workspace must be 8-byte aligned");
  STDADK_REQUIRE(!misaligned(first, 4) && !misaligned(idx_out, 4), STDADK_E_ALIGN,
                 "kmeanspp: first and idx_out must be 4-byte aligned");
  const size_t ub = k > 1 ? (size_t)runs * (size_t)(k - 1) * (size_t)L * sizeof(double) : 0;
  const ByteRange in[] = {{X, (size_t)n * 2 * sizeof(double)}, {first, (size_t)runs * sizeof(int32_t)}, {u, ub}},
                  out[] = {{idx_out, (size_t)runs * k * sizeof(int32_t)}, {pot_out, (size_t)runs * sizeof(double)},
                           {workspace, need}};
  if (int rc = check_no_alias("kmeanspp", out, in, "")) return rc;
  hipStream_t st = (hipStream_t)stream;
  double *dws = (double *)workspace;
  const int64_t per = ceil_div(n, KPP_T);
#define KPP_GO(ROWS) return kpp_launch<ROWS>(X, n, k, runs, L, first, u, idx_out, pot_out, dws, st)
  if (per <= 1) KPP_GO(RegRows<1>);
  if (per <= 2) KPP_GO(RegRows<2>);
  if (per <= 4) KPP_GO(RegRows<4>);
  if (per <= 7) KPP_GO(RegRows<7>);
  if (per <= KPP_MAX_R) KPP_GO(RegRows<KPP_MAX_R>);
  KPP_GO(MemRows);
#undef KPP_GO
}
