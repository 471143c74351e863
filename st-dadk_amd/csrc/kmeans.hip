// One iteration of size-constrained (balanced) k-means in two dimensions (stdadk_kmeans_balanced_iter_f64, see
// include/stdadk.h): the EXACT constrained assignment on the centres given, then the means of the clusters.
//
// The costs c_ij = (x_i - mu_jx)^2 + (y_i - mu_jy)^2 are float64, every operation rounded once (sq_dist_f64 of
// f64_block.h, so that a host restatement forms the same bits).  The assignment works on q_ij = rint(c_ij 2^s), the
// costs on one binary grid of spacing 2^-s <= max c 2^-51 held as 64-bit integers: path sums are then exact, and a
// cycle of exact weight 0 -- duplicated points produce them all the time -- can never round to a negative one and
// keep Bellman-Ford from settling.  An assignment optimal for q is within n max c 2^-51 of the optimum for c.
//
// Launches, in order:
//   km_point_kernel<false>  one thread per point, the centres through LDS in tiles of KM_KT: max_j c_ij, the
//                           workgroup's maximum as one partial.
//   km_scale_kernel         ONE workgroup: the maximum of the partials, s = 52 - exponent.
//   km_q_kernel             one thread per (i, j): q_ij to the workspace, coalesced.
//   km_point_kernel<true>   the same walk as the first: the nearest centre under q (lowest j on a tie) to labels.
//   km_balance_kernel       ONE workgroup of KM_AT threads: member lists, counts cnt_j, targets f_j = clamp(cnt_j, lo,
//                           hi), imbalances; then successive shortest paths on the dense graph of the k clusters and a
//                           sink T, one unit per path, from the nearest-centre assignment (an optimal pseudo-flow) to a
//                           feasible one, which is therefore the optimum.  w(a -> b) = min over the members i of a of
//                           q_ib - q_ia with the lowest such i remembered; w(a -> T) = 0 while f_a < hi; w(T -> b) = 0
//                           while f_b > lo.  Bellman-Ford in synchronous rounds, one node per thread, reading only the
//                           predecessors that moved in the round before (a short list: scanning a flag per node made a
//                           round cost k LDS round trips); the lowest predecessor wins a tie.  The nearest deficit
//                           node by two integer minima; thread 0 walks the predecessors back and applies the path; the
//                           rows of w of the clusters on the path are formed again by all threads.
//   km_mean_kernel          workgroup j: the mean of the members of j, points in index order (thread t takes i = t mod
//                           KM_T), then a fixed tree (block_sum_f64; the maxima go through block_max_f64).
//   km_finish_kernel        ONE workgroup: inertia = sum_i c(x_i, mu_labels[i]), shift = sum_j |mu_out_j - mu_j|^2.
// Every loop is bounded: augmentations by the total surplus (<= n), Bellman-Ford rounds by k + 1, the walk back by
// k + 1; a bound hit writes status[0] != 0 and stops.  No workgroup waits on another.  No float atomics; the integer
// atomics that hand out member slots decide only the ORDER of a member list, and every minimum over a list breaks
// ties by point index, so the same call gives the same bits.
#include "f64_block.h"

namespace stdadk {

constexpr int KM_T = 256;                  // threads = points per workgroup of the point kernels; threads of the others
constexpr int KM_KT = 256;                 // centres per LDS tile of km_point_kernel
constexpr int KM_AT = 1024;                // threads of km_balance_kernel: one per node of the graph
constexpr int KM_MAX_K = 1023;             // k clusters + the sink <= KM_AT
constexpr long long KM_INF = 1ll << 62;    // "no arc" / "not reached"; real path sums stay below (k + 1) 2^52 < 2^62
static_assert(KM_MAX_K + 1 <= KM_AT && KM_KT == KM_T, "one node per thread; one staged centre per thread");

enum { KM_OK = 0, KM_AUGMENTATIONS = 1, KM_NEGATIVE_CYCLE = 2, KM_NO_DEFICIT = 3, KM_PRED_CYCLE = 4, KM_BAD_ARC = 5 };

__device__ __forceinline__ long long km_quant(double c, int sh) { return llrint(ldexp(c, sh)); }

// NEAREST = false: the workgroup's max c to part[blockIdx.x].  NEAREST = true: labels[i] = argmin_j q_ij.
template <bool NEAREST>
__global__ __launch_bounds__(KM_T) void km_point_kernel(const double *__restrict__ X, int n, int k,
                                                        const double *__restrict__ mu, const int *__restrict__ shift,
                                                        double *__restrict__ part, int *__restrict__ labels) {
  __shared__ double cen[KM_KT][2];
  __shared__ double red[KM_T];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * KM_T + tid;
  const bool live = i < n;
  const double x = live ? X[2 * (size_t)i] : 0.0, y = live ? X[2 * (size_t)i + 1] : 0.0;
  const int sh = NEAREST ? shift[0] : 0;
  double cmax = 0.0;
  long long qbest = KM_INF;
  int jbest = 0;
  for (int j0 = 0; j0 < k; j0 += KM_KT) {
    const int nt = k - j0 < KM_KT ? k - j0 : KM_KT;
    __syncthreads();
    if (tid < nt) {
      cen[tid][0] = mu[2 * (j0 + tid)];
      cen[tid][1] = mu[2 * (j0 + tid) + 1];
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const double c = sq_dist_f64(x, y, cen[t][0], cen[t][1]);
      if (NEAREST) {
        const long long q = km_quant(c, sh);
        if (q < qbest) {
          qbest = q;
          jbest = j0 + t;
        }
      } else {
        cmax = c > cmax ? c : cmax;
      }
    }
  }
  if (NEAREST) {
    if (live) labels[i] = jbest;
  } else {
    const double wmax = block_max_f64<KM_T>(red, live ? cmax : 0.0);
    if (tid == 0) part[blockIdx.x] = wmax;
  }
}

__global__ __launch_bounds__(KM_T) void km_scale_kernel(const double *__restrict__ part, int nblk,
                                                        int *__restrict__ shift) {
  __shared__ double red[KM_T];
  const int tid = threadIdx.x;
  double m = 0.0;
  for (int b = tid; b < nblk; b += KM_T) m = part[b] > m ? part[b] : m;
  m = block_max_f64<KM_T>(red, m);
  if (tid == 0) {
    int e = 0;
    if (m > 0.0) frexp(m, &e);
    shift[0] = m > 0.0 ? 52 - e : 0;                 // max c 2^s in [2^51, 2^52)
  }
}

__global__ __launch_bounds__(KM_T) void km_q_kernel(const double *__restrict__ X, int n, int k,
                                                    const double *__restrict__ mu, const int *__restrict__ shift,
                                                    long long *__restrict__ q) {
  const int e = blockIdx.x * KM_T + threadIdx.x;         // n k < 2^31 (km_sizes_ok)
  if (e >= n * k) return;
  const int i = e / k, j = e - i * k;
  q[e] = km_quant(sq_dist_f64(X[2 * (size_t)i], X[2 * (size_t)i + 1], mu[2 * j], mu[2 * j + 1]), shift[0]);
}

struct KmBalanceShared {
  long long dist[2][KM_AT];
  long long redv[KM_AT];
  int redi[KM_AT];
  int pred[KM_AT];
  int cnt[KM_AT], f[KM_AT], imb[KM_AT];
  int path[KM_AT];
  int front[3][KM_AT];               // the nodes whose distance moved in a round, three lists in rotation
  int nfront[3];
  unsigned long long sink_key;       // distance of the nearest deficit node, biased to unsigned
  int sink;
  int need, len, code;
};

// Row a of w again: w[a][b] = min over the members i of a of q[i][b] - q[i][a] and the lowest such i, for every b != a;
// KM_INF for an empty cluster.  Thread (b, s) = (tid % KC, tid / KC) takes the members s, s + S, ...; a tree over s.
__device__ __forceinline__ void km_row(KmBalanceShared &sh, int a, int n, int k, int KC, int S,
                                       const long long *__restrict__ q, const int *mem, long long *w, int *arg) {
  const int tid = threadIdx.x;
  const int b = tid & (KC - 1), s = tid / KC;
  const int m = sh.cnt[a];
  long long best = KM_INF;
  int bi = 0x7fffffff;
  if (b < k && b != a) {
    const int *lst = mem + (size_t)a * n;
    // four members in flight: one workgroup on one compute unit hides the latency of these dependent loads (slot ->
    // point -> two costs) only by issuing them side by side
    for (int t = s; t < m; t += 4 * S) {
      int i[4];
      long long d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) i[u] = t + u * S < m ? lst[t + u * S] : -1;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        d[u] = i[u] >= 0 ? q[(size_t)i[u] * k + b] - q[(size_t)i[u] * k + a] : KM_INF;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i[u] >= 0 && (d[u] < best || (d[u] == best && i[u] < bi))) {
          best = d[u];
          bi = i[u];
        }
    }
  }
  sh.redv[tid] = best;
  sh.redi[tid] = bi;
  __syncthreads();
  for (int o = S / 2; o > 0; o >>= 1) {
    if (s < o) {
      const long long d = sh.redv[tid + o * KC];
      const int i = sh.redi[tid + o * KC];
      if (d < sh.redv[tid] || (d == sh.redv[tid] && i < sh.redi[tid])) {
        sh.redv[tid] = d;
        sh.redi[tid] = i;
      }
    }
    __syncthreads();
  }
  if (s == 0 && b < k) {
    w[(size_t)a * k + b] = sh.redv[tid];
    arg[(size_t)a * k + b] = sh.redi[tid];
  }
  __syncthreads();
}

__global__ __launch_bounds__(KM_AT) void km_balance_kernel(int n, int k, int lo, int hi,
                                                           const long long *__restrict__ q, int *labels, long long *w,
                                                           int *arg, int *mem, int *pos, int *status) {
  // w, arg, mem, pos and labels are written by some threads and read by others across barriers: no __restrict__
  __shared__ KmBalanceShared sh;
  const int tid = threadIdx.x;
  const int T = k, K1 = k + 1;
  int KC = 1;
  while (KC < k) KC <<= 1;
  const int S = KM_AT / KC;

  if (tid < K1) sh.cnt[tid] = 0;
  if (tid == 0) sh.code = KM_OK;
  __syncthreads();
  for (int i = tid; i < n; i += KM_AT) {
    const int a = labels[i];
    const int slot = atomicAdd(&sh.cnt[a], 1);
    mem[(size_t)a * n + slot] = i;
    pos[i] = slot;
  }
  __syncthreads();
  if (tid < k) {
    const int c = sh.cnt[tid];
    sh.f[tid] = c < lo ? lo : (c > hi ? hi : c);
    sh.imb[tid] = c - sh.f[tid];
  }
  __syncthreads();
  if (tid == 0) {
    int sumf = 0, need = 0;
    for (int j = 0; j < k; ++j) {
      sumf += sh.f[j];
      need += sh.imb[j] > 0 ? sh.imb[j] : 0;
    }
    sh.imb[T] = sumf - n;
    sh.f[T] = 0;
    need += sumf - n > 0 ? sumf - n : 0;
    sh.need = need;                                  // = max(total surplus, total deficit) <= n
    if (need > n) sh.code = KM_AUGMENTATIONS;
  }
  __syncthreads();
  const int need = sh.code == KM_OK ? sh.need : 0;
  int aug = 0;
  if (need > 0)
    for (int a = 0; a < k; ++a) km_row(sh, a, n, k, KC, S, q, mem, w, arg);

  while (aug < need) {
    // ---- Bellman-Ford from every surplus node, synchronous rounds ----
    // Round r reads the list r % 3 of the nodes that moved in the round before, appends the nodes it moves to the list
    // (r + 1) % 3 and thread 0 empties the list (r + 2) % 3, which no thread touches in this round.  The slots of a list
    // are handed out by an integer atomic, so its order is arbitrary: a tie between two predecessors of the same round
    // goes to the lower index explicitly; against the distance of earlier rounds only a strictly smaller one wins.
    int cur = 0;
    if (tid < 3) sh.nfront[tid] = 0;
    if (tid == 0) {
      sh.sink_key = ~0ull;
      sh.sink = 0x7fffffff;
    }
    __syncthreads();
    if (tid < K1) {
      const bool src = sh.imb[tid] > 0;
      sh.dist[0][tid] = src ? 0 : KM_INF;
      sh.pred[tid] = -1;
      if (src) sh.front[0][atomicAdd(&sh.nfront[0], 1)] = tid;
    }
    __syncthreads();
    bool settled = false;
    for (int rnd = 0; rnd <= K1; ++rnd) {
      const int nxt = cur ^ 1, lr = rnd % 3, lw = (rnd + 1) % 3;
      if (tid == 0) sh.nfront[(rnd + 2) % 3] = 0;
      if (tid < K1) {
        long long best = sh.dist[cur][tid];
        int bp = sh.pred[tid];
        bool moved = false;
        const int nf = sh.nfront[lr];
        for (int e = 0; e < nf; ++e) {
          const int a = sh.front[lr][e];
          long long wv = 0;
          bool arc;
          if (tid == T) {
            arc = a != T && sh.f[a] < hi;
          } else if (a == T) {
            arc = sh.f[tid] > lo;
          } else {
            wv = w[(size_t)a * k + tid];
            arc = wv < KM_INF;
          }
          if (!arc) continue;
          const long long cand = sh.dist[cur][a] + wv;
          if (cand < best || (moved && cand == best && a < bp)) {
            best = cand;
            bp = a;
            moved = true;
          }
        }
        sh.dist[nxt][tid] = best;
        sh.pred[tid] = bp;
        if (moved) sh.front[lw][atomicAdd(&sh.nfront[lw], 1)] = tid;
      }
      __syncthreads();
      cur = nxt;
      if (sh.nfront[lw] == 0) {
        settled = true;
        break;
      }
    }
    // ---- the nearest deficit node, the lowest index among equals: two integer minima over the nodes ----
    const bool deficit = settled && tid < K1 && sh.imb[tid] < 0 && sh.dist[cur][tid] < KM_INF;
    const unsigned long long key = deficit ? (unsigned long long)(sh.dist[cur][tid] + KM_INF) : ~0ull;
    if (deficit) atomicMin(&sh.sink_key, key);
    __syncthreads();
    if (deficit && key == sh.sink_key) atomicMin(&sh.sink, tid);
    __syncthreads();
    // ---- thread 0: the walk back from it, the path applied ----
    if (tid == 0) {
      int code = settled ? KM_OK : KM_NEGATIVE_CYCLE, len = 0;
      if (code == KM_OK) {
        const int v = sh.sink < K1 ? sh.sink : -1;
        if (v < 0) code = KM_NO_DEFICIT;
        for (int u = v; code == KM_OK && u >= 0; u = sh.pred[u]) {
          if (len >= K1) {
            code = KM_PRED_CYCLE;
            break;
          }
          sh.path[len++] = u;                        // sink first, source last
        }
      }
      if (code == KM_OK) {
        sh.imb[sh.path[0]] += 1;
        sh.imb[sh.path[len - 1]] -= 1;
        for (int p = len - 1; p > 0; --p) {
          const int u = sh.path[p], v = sh.path[p - 1];
          if (v == T) {
            sh.f[u] += 1;
          } else if (u == T) {
            sh.f[v] -= 1;
          } else {                                   // the remembered point of (u, v) moves from u to v
            const int i = arg[(size_t)u * k + v];
            if (i < 0 || i >= n || sh.cnt[u] < 1) {      // never on a path of finite length; checked before any index
              code = KM_BAD_ARC;
              break;
            }
            int *lu = mem + (size_t)u * n, *lv = mem + (size_t)v * n;
            const int slot = pos[i], last = lu[sh.cnt[u] - 1];
            lu[slot] = last;
            pos[last] = slot;
            sh.cnt[u] -= 1;
            lv[sh.cnt[v]] = i;
            pos[i] = sh.cnt[v];
            sh.cnt[v] += 1;
            labels[i] = v;
          }
        }
      }
      sh.code = code;
      sh.len = len;
    }
    __syncthreads();
    if (sh.code != KM_OK) break;
    ++aug;
    const int len = sh.len;
    for (int p = 0; p < len; ++p) {
      const int a = sh.path[p];
      if (a != T) km_row(sh, a, n, k, KC, S, q, mem, w, arg);
    }
  }
  if (tid == 0) {
    status[0] = sh.code;
    status[1] = aug;
  }
}

__global__ __launch_bounds__(KM_T) void km_mean_kernel(const double *__restrict__ X, int n,
                                                       const int *__restrict__ labels, const double *__restrict__ mu,
                                                       double *__restrict__ mu_out) {
  __shared__ double red[KM_T];
  const int j = blockIdx.x, tid = threadIdx.x;
  double sx = 0.0, sy = 0.0, c = 0.0;
  for (int i = tid; i < n; i += KM_T)
    if (labels[i] == j) {
      sx += X[2 * (size_t)i];
      sy += X[2 * (size_t)i + 1];
      c += 1.0;
    }
  sx = block_sum_f64<KM_T>(red, sx);
  sy = block_sum_f64<KM_T>(red, sy);
  c = block_sum_f64<KM_T>(red, c);
  if (tid == 0) {                                    // c >= lo >= 1 unless the assignment stopped on a bound (status)
    mu_out[2 * j] = c > 0.0 ? sx / c : mu[2 * j];
    mu_out[2 * j + 1] = c > 0.0 ? sy / c : mu[2 * j + 1];
  }
}

__global__ __launch_bounds__(KM_T) void km_finish_kernel(const double *__restrict__ X, int n, int k,
                                                         const int *__restrict__ labels, const double *__restrict__ mu,
                                                         const double *__restrict__ mu_out, double *__restrict__ stats) {
  __shared__ double red[KM_T];
  const int tid = threadIdx.x;
  double a = 0.0, s = 0.0;
  for (int i = tid; i < n; i += KM_T) {
    const int j = labels[i];
    a += sq_dist_f64(X[2 * (size_t)i], X[2 * (size_t)i + 1], mu[2 * j], mu[2 * j + 1]);
  }
  for (int j = tid; j < k; j += KM_T) s += sq_dist_f64(mu_out[2 * j], mu_out[2 * j + 1], mu[2 * j], mu[2 * j + 1]);
  a = block_sum_f64<KM_T>(red, a);
  s = block_sum_f64<KM_T>(red, s);
  if (tid == 0) {
    stats[0] = a;
    stats[1] = s;
  }
}

static inline bool km_sizes_ok(int64_t n, int32_t k) {
  return n >= 1 && k >= 1 && k <= KM_MAX_K && n * (int64_t)k < (1ll << 31);
}

struct KmLayout {
  size_t q, w, part, shift, arg, mem, pos, bytes;    // byte offsets into the workspace
};
static inline KmLayout km_layout(int64_t n, int32_t k) {
  KmLayout L;
  size_t o = 0;
  L.q = o, o += (size_t)n * k * 8;
  L.w = o, o += (size_t)k * k * 8;
  L.part = o, o += (size_t)ceil_div(n, KM_T) * 8;
  L.shift = o, o += 8;
  L.arg = o, o += (size_t)k * k * 4;
  L.mem = o, o += (size_t)k * n * 4;
  L.pos = o, o += (size_t)n * 4;
  L.bytes = align_up(o, 8);
  return L;
}

}  // namespace stdadk

using namespace stdadk;

// workspace: q [n][k] and w [k][k] (int64), the maximum's partials [ceil(n / KM_T)], s, arg [k][k], the member lists
// [k][n] and the member slots [n] (int32)
extern "C" size_t stdadk_kmeans_workspace_bytes(int64_t n, int32_t k) {
  if (!km_sizes_ok(n, k)) return 0;
  return km_layout(n, k).bytes;
}

extern "C" int stdadk_kmeans_balanced_iter_f64(const double *X, int64_t n, int32_t k, const double *mu, int32_t lo,
                                               int32_t hi, double *mu_out, int32_t *labels, double *stats,
                                               int32_t *status, void *workspace, size_t workspace_bytes,
                                               stdadk_stream_t stream) {
  STDADK_REQUIRE(n >= 1 && k >= 1 && k <= KM_MAX_K, STDADK_E_ARG, "kmeans_balanced_iter: n=%lld, k=%d outside n >= 1, 1..%d",
                 (long long)n, k, KM_MAX_K);
  STDADK_REQUIRE(n * (int64_t)k < (1ll << 31), STDADK_E_ARG, "kmeans_balanced_iter: n k = %lld x %d is 2^31 or more",
                 (long long)n, k);
  STDADK_REQUIRE(X && mu && mu_out && labels && stats && status && workspace, STDADK_E_ARG,
                 "kmeans_balanced_iter: NULL pointer");
  STDADK_REQUIRE(k <= n, STDADK_E_SHAPE, "kmeans_balanced_iter: k=%d clusters on n=%lld points", k, (long long)n);
  STDADK_REQUIRE(lo >= 1 && lo <= hi, STDADK_E_SHAPE, "kmeans_balanced_iter: bounds lo=%d, hi=%d need 1 <= lo <= hi", lo, hi);
  STDADK_REQUIRE((int64_t)lo * k <= n, STDADK_E_SHAPE, "kmeans_balanced_iter: lo k = %d x %d exceeds n=%lld", lo, k,
                 (long long)n);
  STDADK_REQUIRE((int64_t)hi * k >= n, STDADK_E_SHAPE, "kmeans_balanced_iter: hi k = %d x %d is below n=%lld", hi, k,
                 (long long)n);
  const KmLayout L = km_layout(n, k);
  if (int rc = check_workspace("kmeans_balanced_iter", workspace, workspace_bytes, L.bytes, "stdadk_kmeans_workspace_bytes"))
    return rc;
  const size_t kb = (size_t)k * 2 * sizeof(double);
  const ByteRange in[] = {{X, (size_t)n * 2 * sizeof(double)}, {mu, kb}},
                  out[] = {{mu_out, kb}, {labels, (size_t)n * sizeof(int32_t)}, {stats, 2 * sizeof(double)},
                           {status, 2 * sizeof(int32_t)}, {workspace, L.bytes}};
  if (int rc = check_no_alias("kmeans_balanced_iter", out, in, " (the caller ping-pongs two sets of centres)")) return rc;
  char *base = (char *)workspace;
  long long *q = (long long *)(base + L.q), *w = (long long *)(base + L.w);
  double *part = (double *)(base + L.part);
  int *shift = (int *)(base + L.shift), *arg = (int *)(base + L.arg), *mem = (int *)(base + L.mem),
      *pos = (int *)(base + L.pos);
  const int nblk = (int)ceil_div(n, KM_T), ni = (int)n;
  hipStream_t st = (hipStream_t)stream;
  STDADK_LAUNCH_NAMED("km_max_kernel", km_point_kernel<false>, dim3((unsigned)nblk), dim3(KM_T), 0, st, X, ni, (int)k, mu,
                      (const int *)shift, part, (int *)labels);
  STDADK_CHECK_LAUNCH("km_max");
  STDADK_LAUNCH(km_scale_kernel, dim3(1), dim3(KM_T), 0, st, (const double *)part, nblk, shift);
  STDADK_CHECK_LAUNCH("km_scale");
  STDADK_LAUNCH(km_q_kernel, dim3((unsigned)ceil_div(n * k, KM_T)), dim3(KM_T), 0, st, X, ni, (int)k, mu,
                (const int *)shift, q);
  STDADK_CHECK_LAUNCH("km_q");
  STDADK_LAUNCH_NAMED("km_nearest_kernel", km_point_kernel<true>, dim3((unsigned)nblk), dim3(KM_T), 0, st, X, ni, (int)k,
                      mu, (const int *)shift, part, (int *)labels);
  STDADK_CHECK_LAUNCH("km_nearest");
  STDADK_LAUNCH(km_balance_kernel, dim3(1), dim3(KM_AT), 0, st, ni, (int)k, (int)lo, (int)hi, (const long long *)q,
                (int *)labels, w, arg, mem, pos, (int *)status);
  STDADK_CHECK_LAUNCH("km_balance");
  STDADK_LAUNCH(km_mean_kernel, dim3((unsigned)k), dim3(KM_T), 0, st, X, ni, (const int *)labels, mu, mu_out);
  STDADK_CHECK_LAUNCH("km_mean");
  STDADK_LAUNCH(km_finish_kernel, dim3(1), dim3(KM_T), 0, st, X, ni, (int)k, (const int *)labels, mu,
                (const double *)mu_out, stats);
  STDADK_CHECK_LAUNCH("km_finish");
  return 0;
}
