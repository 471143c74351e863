// A6-A8: dense MLP forward / backward around the fp32 MFMA GEMM, plus the fused MSE loss.
//
//   forward  (stnf/models/st_interp.py:656-690,880):  per hidden layer
//       z = a_prev W^T (+b)          split-K MFMA GEMM -> partial slabs
//       LN -> ReLU -> Dropout        one wave per row; sums the slabs, adds the bias, saves xhat/rstd
//   backward (scripts/train_st_interp.py:693): per hidden layer, last to first
//       dz, partial column sums      one wave per row (LN backward, ReLU/dropout mask recomputed)
//       dgamma, dbeta, db            column-sum reduction of the per-workgroup partials
//       dW = dz^T a_prev             split-K (over the batch) MFMA GEMM -> slabs -> sum
//       da_prev = dz W               MFMA GEMM (skipped for the first layer: knots are buffers)
#include "common.h"
#include "gemm_f32.h"
#include "window.h"
#include "tail.h"
#include "optim.h"
#include "bin_body.h"
#include "knots.h"
#include "step_finish.h"
#include "basis.h"
#include "loss.h"

#include <stdlib.h>

namespace stdadk {

constexpr int ROW_T = 256;        // threads of the row kernels: 4 waves = 4 rows in flight
constexpr int MAX_CPL = 16;       // columns per lane => hidden width <= 1024

// rows per workgroup of the backward row kernels: 16 up to B = 8192, then <= 512 workgroups
static int bwd_rows(int64_t B) {
  if (B <= 8192) return 16;
  return (int)(ceil_div(ceil_div(B, 512), 4) * 4);
}

// ---------------------------------------------------------------------------------------------
// workspace plan (offsets in floats; every sub-buffer starts on a 256-byte boundary)
// ---------------------------------------------------------------------------------------------
enum PlanMode { PLAN_MLP = 0, PLAN_STEP_DENSE = 1, PLAN_STEP_WINDOW = 2 };

// rows from which the merged weight-gradient launch also does the reductions (finishing_mode, FinArgs): measured
// per step at 8 192 / 16 384 / 32 768 / 65 536 rows: +4 / 0 / -9 / -17 us against the reductions launch
constexpr int64_t FIN_FULL_MIN_ROWS = 49152;

struct Plan {
  int L;
  int64_t B;
  size_t xhat[STDADK_MAX_HIDDEN], rstd[STDADK_MAX_HIDDEN], act[STDADK_MAX_HIDDEN];
  size_t slab, slab_floats;
  size_t dA, dZ;            // [B][hmax] each
  size_t part, part_floats; // column-sum partials
  size_t dZl[STDADK_MAX_HIDDEN], partl[STDADK_MAX_HIDDEN];   // fused tail: per-layer dZ and partials
  // step-level buffers
  size_t feats; int64_t ldf;           // dense: materialised features
  size_t bw_exp, kpart; int kslabs;    // learnable knots: exp(log_bw) [Ks], per-slab knot partials
  size_t halo;                         // learnable knots, window path: per-level partial maxima of the candidate reach
  size_t kcs, kperm, kperm_tmp, reach; // scattered knots, window path: per-level cell lists of the knots (knot_bins)
  size_t psi; int ld_psi;              // window: temporal basis [B][ld_psi]
  size_t ypred, dY;                    // [B*Q]
  size_t keys, hist, cursor, cell_start, perm_tmp, perm, xs, ys, ts, y_s, X_s;
  int G;
  size_t fin_cnt, fin_slots; int fin_cap;   // window path: arrival counters / squared-norm slots of the merged dW launch
  size_t total_floats;
};

static void make_plan(const stdadk_mlp_desc *d, int64_t B, Plan *p, int mode = PLAN_MLP, int p_cov = 0,
                      int Kt = 0, int64_t Ks_learn = 0, int64_t Ks_scattered = 0, int n_levels = 0,
                      int64_t Ks_window = 0) {
  p->L = d->n_hidden;
  p->B = B;
  size_t off = 0;
  auto take = [&](size_t n) {
    size_t o = off;
    off += align_up(n > 0 ? n : 1, 64);
    return o;
  };
  int hmax = d->out_dim;
  size_t slab = 0;
  int prev = d->in_dim;
  for (int l = 0; l < d->n_hidden; ++l) {
    int h = d->hidden[l];
    p->xhat[l] = take((size_t)B * h);
    p->rstd[l] = take((size_t)B);
    p->act[l] = take((size_t)B * h);
    hmax = h > hmax ? h : hmax;
    size_t s;
    if (!(l == 0 && mode == PLAN_STEP_WINDOW)) {
      s = gemm_slab_floats((int)B, h, prev); slab = s > slab ? s : slab;          // forward z
      s = gemm_slab_floats(h, prev, (int)B); slab = s > slab ? s : slab;          // dW  (M=h)
      s = gemm_slab_floats(prev, h, (int)B); slab = s > slab ? s : slab;          // dW^T (layer 0, W0 transposed)
    }
    if (l > 0 || Ks_learn > 0) { s = gemm_slab_floats((int)B, prev, h); slab = s > slab ? s : slab; }  // dA (layer 0: dFeat, learnable knots)
    prev = h;
  }
  {
    size_t s = gemm_slab_floats((int)B, d->out_dim, prev); slab = s > slab ? s : slab;
    s = gemm_slab_floats(d->out_dim, prev, (int)B); slab = s > slab ? s : slab;
    s = gemm_slab_floats((int)B, prev, d->out_dim); slab = s > slab ? s : slab;
  }
  if (mode == PLAN_STEP_WINDOW && d->n_hidden > 0) {
    size_t s = gemm_slab_floats(Kt, d->hidden[0], (int)B); slab = s > slab ? s : slab;
    if (p_cov > 0) { s = gemm_slab_floats(p_cov, d->hidden[0], (int)B); slab = s > slab ? s : slab; }
  }
  {
    // the grouped dW launch of the fused-tail backward keeps every job's slabs alive at once
    auto job_floats = [&](int M, int N) {
      int kps;
      int sp = gemm_pick_splits(M, N, (int)B, &kps, false);
      return (size_t)sp * M * N;
    };
    size_t grouped = 0;
    for (int l = 1; l < d->n_hidden; ++l) grouped += job_floats(d->hidden[l], d->hidden[l - 1]);
    if (mode == PLAN_STEP_WINDOW && d->n_hidden > 0) {
      grouped += job_floats(Kt, d->hidden[0]);
      if (p_cov > 0) grouped += job_floats(p_cov, d->hidden[0]);
    } else if (d->n_hidden > 0) {
      // materialising path, small D: dW0^T = features^T dZ_0 is a split-K product too and joins the group
      int kps;
      if (gemm_pick_splits(d->in_dim, d->hidden[0], (int)B, &kps, false) > 1) grouped += job_floats(d->in_dim, d->hidden[0]);
    }
    slab = grouped > slab ? grouped : slab;
  }
  p->slab_floats = slab;
  p->slab = take(slab);
  p->dA = take((size_t)B * hmax);
  p->dZ = take((size_t)B * hmax);
  int64_t nblk = ceil_div(B, bwd_rows(B));
  p->part_floats = (size_t)nblk * 3 * hmax;
  size_t head = (size_t)nblk * (size_t)d->out_dim * (hmax + 1);
  if (head > p->part_floats) p->part_floats = head;
  {
    const int64_t nb16 = ceil_div(B, TAIL_MIN_ROWS);
    size_t head16 = (size_t)nb16 * (size_t)d->out_dim * (hmax + 1);
    if (head16 > p->part_floats) p->part_floats = head16;
  }
  p->part = take(p->part_floats);
  for (int l = 0; l < d->n_hidden; ++l) {
    p->dZl[l] = take((size_t)B * d->hidden[l]);
    p->partl[l] = take((size_t)ceil_div(B, TAIL_MIN_ROWS) * 3 * d->hidden[l]);
  }
  p->feats = p->psi = p->ypred = p->dY = 0;
  p->ldf = 0; p->ld_psi = 0; p->G = 0;
  if (mode != PLAN_MLP) {
    p->ypred = take((size_t)B * d->out_dim);
    p->dY = take((size_t)B * d->out_dim);
  }
  if (mode == PLAN_STEP_DENSE) {
    p->ldf = (int64_t)align_up((size_t)d->in_dim, 32);
    p->feats = take((size_t)B * p->ldf);
  }
  p->bw_exp = p->kpart = p->halo = 0; p->kslabs = 0;
  if (mode != PLAN_MLP && Ks_learn > 0) {
    // dense: one partial per row slab; window: the wave that owns a knot produces its whole sum
    p->kslabs = mode == PLAN_STEP_DENSE ? knot_slabs(B) : 1;
    p->bw_exp = take((size_t)Ks_learn);
    p->kpart = take((size_t)p->kslabs * 3 * (size_t)Ks_learn);
    p->halo = take((size_t)STDADK_MAX_LEVELS * HALO_SPLIT);
  }
  p->kcs = p->kperm = p->kperm_tmp = p->reach = 0;
  if (mode == PLAN_STEP_WINDOW && Ks_scattered > 0) {
    p->kcs = take((size_t)n_levels * (KNOT_CELLS * KNOT_CELLS + 1));
    p->kperm = take((size_t)Ks_scattered);
    p->kperm_tmp = take((size_t)Ks_scattered);
    p->reach = take(STDADK_MAX_LEVELS);
    if (Ks_learn == 0) p->bw_exp = take(1);      // (fixed scattered knots: no exp table)
  }
  if (mode == PLAN_STEP_WINDOW) {
    p->G = pick_cell_grid(B);
    p->ld_psi = (int)align_up((size_t)(Kt > 0 ? Kt : 1), 4);
    p->psi = take((size_t)B * p->ld_psi);
    size_t nc = (size_t)p->G * p->G + 1;
    p->keys = take(B); p->hist = take(nc); p->cursor = take(nc); p->cell_start = take(nc);
    p->perm_tmp = take(B); p->perm = take(B);
    p->xs = take(B); p->ys = take(B); p->ts = take(B);
    p->y_s = take((size_t)B * d->out_dim);
    p->X_s = take((size_t)B * (p_cov > 0 ? p_cov : 1));
  }
  p->fin_cnt = p->fin_slots = 0; p->fin_cap = 0;
  if (mode == PLAN_STEP_WINDOW) {
    // output tiles + tall reduce workgroups + knot workgroups (at most one per knot + the padding of the
    // XCD-striped order), see FinArgs
    p->fin_cap = FIN_TILES_MAX + 1024 + (int)Ks_window + 64;
    p->fin_cnt = take(FIN_TILES_MAX);
    p->fin_slots = take((size_t)p->fin_cap);
  }
  p->total_floats = off;
}

// ---------------------------------------------------------------------------------------------
// row kernels
// ---------------------------------------------------------------------------------------------
// z[row][c] = sum_s slab[s][row][c] (+ bias[c]); LayerNorm -> ReLU -> Dropout.  One wave per row.
template <bool LN, int CPL>
__global__ __launch_bounds__(ROW_T) void ln_relu_fwd_kernel(
    const float *__restrict__ zsrc, int splits, int64_t slab_stride, const float *__restrict__ bias,
    const float *__restrict__ gamma, const float *__restrict__ beta, float eps, int64_t B, int h,
    float *__restrict__ xhat, float *__restrict__ rstd_out, float *__restrict__ act, float drop_p,
    uint64_t seed, const int *__restrict__ step_dev, int layer, const uint8_t *__restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (ROW_T / 64) + (threadIdx.x >> 6);
  if (row >= B) return;
  if (step_dev) seed += (uint64_t)step_dev[0] * 0x9E3779B97F4A7C15ULL;
  float z[CPL];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    int c = lane + 64 * j;
    z[j] = 0.f;
    if (c < h) {
      float v = bias ? bias[c] : 0.f;
      for (int s = 0; s < splits; ++s) v += zsrc[(int64_t)s * slab_stride + row * h + c];
      z[j] = v;
      sum += v;
    }
  }
  float rs = 1.f, mean = 0.f;
  if (LN) {
    const float inv_h = 1.0f / (float)h;
    mean = wave_sum(sum) * inv_h;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (lane + 64 * j < h) { float d = z[j] - mean; sq += d * d; }
    float var = wave_sum(sq) * inv_h;
    rs = ln_rstd(var, eps);
    if (lane == 0) rstd_out[row] = rs;
  }
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  const uint32_t rowkey = drop_rowkey(seed, layer, row), drop_thr = drop_threshold(drop_p);
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    int c = lane + 64 * j;
    if (c < h) {
      float xh = LN ? (z[j] - mean) * rs : z[j];
      float u = LN ? fmaf(xh, gamma[c], beta[c]) : xh;
      float a = fmaxf(u, 0.f);
      if (drop_p > 0.f) {
        int64_t e = row * h + c;
        bool keep = mask ? (mask[e] != 0) : drop_keep(rowkey, c, drop_thr);
        a = keep ? a * keep_scale : 0.f;
      }
      xhat[row * h + c] = xh;
      act[row * h + c] = a;
    }
  }
}

// Backward of Dropout -> ReLU -> LayerNorm for rows_per_wg rows per workgroup:
//   du = dA * keep/(1-p) * (u > 0);  dgamma += du*xhat;  dbeta += du
//   dz = rstd * (dxh - mean(dxh) - xhat*mean(dxh*xhat)),  dxh = du*gamma;   db += dz
// Column partials go to part[blk][3][h] (dgamma, dbeta, db) and are summed by colsum_kernel.
template <bool LN, int CPL>
__global__ __launch_bounds__(ROW_T) void ln_relu_bwd_kernel(
    const float *__restrict__ dA, const float *__restrict__ xhat, const float *__restrict__ rstd,
    const float *__restrict__ gamma, const float *__restrict__ beta, int64_t B, int h,
    float *__restrict__ dZ, float *__restrict__ part, float drop_p, uint64_t seed,
    const int *__restrict__ step_dev, int layer, const uint8_t *__restrict__ mask, int rows_per_wg) {
  __shared__ float red[3][ROW_T / 64][256];
  if (step_dev) seed += (uint64_t)step_dev[0] * 0x9E3779B97F4A7C15ULL;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  float pg[CPL], pb[CPL], pz[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) pg[j] = pb[j] = pz[j] = 0.f;
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_wg;
  for (int rr = wave; rr < rows_per_wg; rr += ROW_T / 64) {
    const int64_t row = row0 + rr;
    if (row >= B) break;
    float du[CPL], xh[CPL];
    float s1 = 0.f, s2 = 0.f;
    const uint32_t rowkey = drop_rowkey(seed, layer, row), drop_thr = drop_threshold(drop_p);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      int c = lane + 64 * j;
      du[j] = 0.f; xh[j] = 0.f;
      if (c < h) {
        int64_t e = row * h + c;
        float x = xhat[e];
        float u = LN ? fmaf(x, gamma[c], beta[c]) : x;
        float d = dA[e];
        if (drop_p > 0.f) {
          bool keep = mask ? (mask[e] != 0) : drop_keep(rowkey, c, drop_thr);
          d = keep ? d * keep_scale : 0.f;
        }
        d = u > 0.f ? d : 0.f;
        du[j] = d; xh[j] = x;
        if (LN) {
          pg[j] += d * x;
          pb[j] += d;
          float dxh = d * gamma[c];
          s1 += dxh;
          s2 += dxh * x;
        }
      }
    }
    float rs = 1.f, m1 = 0.f, m2 = 0.f;
    if (LN) {
      const float inv_h = 1.0f / (float)h;
      m1 = wave_sum(s1) * inv_h;
      m2 = wave_sum(s2) * inv_h;
      rs = rstd[row];
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      int c = lane + 64 * j;
      if (c < h) {
        float dz = LN ? rs * (du[j] * gamma[c] - m1 - xh[j] * m2) : du[j];
        dZ[row * h + c] = dz;
        pz[j] += dz;
      }
    }
  }
  // cross-wave reduction of the column partials, 256 columns at a time
  float *pbase = part + (int64_t)blockIdx.x * 3 * h;
#pragma unroll
  for (int j0 = 0; j0 < CPL; j0 += 4) {
    if (64 * j0 < h) {   // workgroup-uniform
      __syncthreads();
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        if (j0 + jj < CPL) {
          red[0][wave][lane + 64 * jj] = pg[j0 + jj];
          red[1][wave][lane + 64 * jj] = pb[j0 + jj];
          red[2][wave][lane + 64 * jj] = pz[j0 + jj];
        }
      }
      __syncthreads();
      int c = 64 * j0 + threadIdx.x;   // 256 threads <-> 256 columns
      if (c < h) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          float s = red[q][0][threadIdx.x] + red[q][1][threadIdx.x] + red[q][2][threadIdx.x] + red[q][3][threadIdx.x];
          pbase[q * h + c] = s;
        }
      }
    }
  }
}

// Column sums of per-workgroup partials: out_q[c] = sum_blk part[blk*stride + q*seg + c], q < nseg.
// 64 columns x 4 block-quarters per workgroup, LDS reduction over the quarters.
struct ColsumOut { float *o[3]; };
constexpr int CS_G = 16;   // block-groups per workgroup
__global__ __launch_bounds__(64 * CS_G) void colsum_kernel(const float *__restrict__ part, int64_t nblk,
                                                           int64_t stride, int seg, int nseg,
                                                           ColsumOut out) {
  __shared__ float red[CS_G][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  const int n = seg * nseg;
  float s0 = 0.f, s1 = 0.f;
  if (c < n) {
    int64_t b = ty;
    for (; b + CS_G < nblk; b += 2 * CS_G) {
      s0 += part[b * stride + c];
      s1 += part[(b + CS_G) * stride + c];
    }
    for (; b < nblk; b += CS_G) s0 += part[b * stride + c];
  }
  red[ty][tx] = s0 + s1;
  __syncthreads();
  if (ty == 0 && c < n) {
    float v = 0.f;
#pragma unroll
    for (int g = 0; g < CS_G; ++g) v += red[g][tx];
    int q = c / seg;
    out.o[q][c - q * seg] = v;
  }
}

// Output layer for small Q: y[row][q] = a[row,:] . W[q,:] + b[q].  One wave per row.
constexpr int HEAD_MAXQ = 8;
__global__ __launch_bounds__(ROW_T) void head_fwd_kernel(const float *__restrict__ a, int64_t B, int h,
                                                         const float *__restrict__ W,
                                                         const float *__restrict__ b, int Q,
                                                         float *__restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (ROW_T / 64) + (threadIdx.x >> 6);
  if (row >= B) return;
  float acc[HEAD_MAXQ];
#pragma unroll
  for (int q = 0; q < HEAD_MAXQ; ++q) acc[q] = 0.f;
  for (int c = lane; c < h; c += 64) {
    float v = a[row * h + c];
#pragma unroll
    for (int q = 0; q < HEAD_MAXQ; ++q)
      if (q < Q) acc[q] = fmaf(v, W[q * h + c], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < HEAD_MAXQ; ++q) {
    if (q < Q) {
      float s = wave_sum(acc[q]);
      if (lane == 0) y[row * Q + q] = s + b[q];
    }
  }
}

// Backward of the small-Q output layer for rows_per_wg rows per workgroup:
//   dA[row][c] = sum_q dY[row][q] W[q][c];  partial dW[q][c] = sum_rows dY[row][q] a[row][c];
//   partial db[q] = sum_rows dY[row][q].   part[blk][q][h+1] (last column = db).
__global__ __launch_bounds__(ROW_T) void head_bwd_kernel(const float *__restrict__ a,
                                                         const float *__restrict__ dY, int64_t B,
                                                         int h, const float *__restrict__ W, int Q,
                                                         float *__restrict__ dA,
                                                         float *__restrict__ part, int rows_per_wg) {
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_wg;
  const int nrow = (int)min((int64_t)rows_per_wg, B - row0);
  extern __shared__ float sdy[];   // [rows_per_wg][Q]
  for (int i = threadIdx.x; i < nrow * Q; i += ROW_T) sdy[i] = dY[row0 * Q + i];
  __syncthreads();
  float *pbase = part + (int64_t)blockIdx.x * Q * (h + 1);
  for (int c = threadIdx.x; c < h; c += ROW_T) {
    float w[HEAD_MAXQ], pw[HEAD_MAXQ];
#pragma unroll
    for (int q = 0; q < HEAD_MAXQ; ++q) { w[q] = q < Q ? W[q * h + c] : 0.f; pw[q] = 0.f; }
    for (int r = 0; r < nrow; ++r) {
      float av = a[(row0 + r) * h + c];
      float d = 0.f;
#pragma unroll
      for (int q = 0; q < HEAD_MAXQ; ++q)
        if (q < Q) { float g = sdy[r * Q + q]; d = fmaf(g, w[q], d); pw[q] = fmaf(g, av, pw[q]); }
      dA[(row0 + r) * h + c] = d;
    }
#pragma unroll
    for (int q = 0; q < HEAD_MAXQ; ++q)
      if (q < Q) pbase[q * (h + 1) + c] = pw[q];
  }
  if (threadIdx.x < Q) {
    float s = 0.f;
    for (int r = 0; r < nrow; ++r) s += sdy[r * Q + threadIdx.x];
    pbase[threadIdx.x * (h + 1) + h] = s;
  }
}

// sum the head partials [blk][Q][h+1] and split them into dW[Q][h] and db[Q]
__global__ __launch_bounds__(64 * CS_G) void head_reduce_kernel(const float *__restrict__ part, int64_t nblk,
                                                                int Q, int h, float *__restrict__ dW,
                                                                float *__restrict__ db) {
  __shared__ float red[CS_G][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + tx;
  const int n = Q * (h + 1);
  float s = 0.f;
  if (i < n)
    for (int64_t b = ty; b < nblk; b += CS_G) s += part[b * n + i];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && i < n) {
    float v = 0.f;
#pragma unroll
    for (int g = 0; g < CS_G; ++g) v += red[g][tx];
    int q = i / (h + 1), c = i - q * (h + 1);
    if (c < h) dW[q * h + c] = v; else db[q] = v;
  }
}

__global__ void mse_kernel(const float *__restrict__ yp, const float *__restrict__ y, int64_t n,
                           float scale, float *__restrict__ dY, float *__restrict__ loss_sum) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float d = yp[i] - y[i];
    acc = fmaf(d, d, acc);
    if (dY) dY[i] = 2.0f * d * scale;
  }
  if (loss_sum) {
    __shared__ float red[4];
    float s = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss_sum, red[0] + red[1] + red[2] + red[3]);
  }
}

// out[i][q] = in[perm[i]][q]
__global__ void gather_rows_kernel(const float *__restrict__ in, const int *__restrict__ perm, int B, int Q,
                                   float *__restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * Q) return;
  int r = i / Q, q = i - r * Q;
  out[i] = in[(int64_t)perm[r] * Q + q];
}

// ---------------------------------------------------------------------------------------------
// host-side orchestration
// ---------------------------------------------------------------------------------------------
static int check_desc(const stdadk_mlp_desc *d) {
  STDADK_REQUIRE(d != nullptr, STDADK_E_ARG, "mlp: desc is NULL");
  STDADK_REQUIRE(d->n_hidden >= 0 && d->n_hidden <= STDADK_MAX_HIDDEN, STDADK_E_ARG,
                 "mlp: n_hidden %d out of range", d->n_hidden);
  STDADK_REQUIRE(d->in_dim > 0 && d->out_dim > 0, STDADK_E_ARG, "mlp: in_dim/out_dim must be > 0");
  for (int l = 0; l < d->n_hidden; ++l)
    STDADK_REQUIRE(d->hidden[l] > 0 && d->hidden[l] <= 64 * MAX_CPL, STDADK_E_SHAPE,
                   "mlp: hidden[%d]=%d unsupported (1..%d)", l, d->hidden[l], 64 * MAX_CPL);
  STDADK_REQUIRE(d->dropout_p >= 0.f && d->dropout_p < 1.f, STDADK_E_ARG, "mlp: dropout_p out of range");
  return 0;
}

// the default objective: plain MSE against y [B,Q] (y_cols 0 = Q), every quantile level 0.5
static const LossDev LOSS_PLAIN_MSE = {STDADK_LOSS_MSE, 0, {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f}, 0.f, 1};

// One description of a training step call: what the public doors take positionally, by name
struct StepCall {
  const stdadk_basis_desc *b = nullptr;
  const stdadk_mlp_desc *d = nullptr;
  const stdadk_mlp_tensors *P = nullptr, *G = nullptr;
  const float *coords = nullptr, *t = nullptr, *X = nullptr, *y = nullptr;   // the batch: these arrays, or with `idx`
  const int64_t *idx = nullptr;                                              // (window path) their rows idx[0..B)
  int64_t B = 0;
  float grad_scale = 0.f;
  const stdadk_loss_desc *loss = nullptr;
  float *loss_sum = nullptr, *y_pred = nullptr;
  void *workspace = nullptr;
  size_t workspace_bytes = 0;
  uint64_t drop_seed = 0;
  const int32_t *step_dev = nullptr;
  int32_t flags = 0;
  stdadk_stream_t stream = nullptr, aux_stream = nullptr;
};
// StepRide: what the one-call step lets ride along with its launches -- squared-norm partials of the gradient with the step
// counter their launch advances, the next batch for the merged dW launch to bin; StepOut: where the partials went (NULL:
// no launch left them) and whether that batch is binned
struct StepRide {
  float *gradsq_parts = nullptr; int32_t *step_inc = nullptr; const BinSmallArgs *bin_next = nullptr;
  // two parameter groups (stdadk_train_step_knots_f32): the knot finish rides in the step's finishing launch, which
  // leaves the knot group's partials in knot_sq (NULL: unclipped) and advances finish_inc (step_inc stays NULL then)
  bool knots = false;
  const stdadk_knot_train *kt = nullptr;
  float *d_centers = nullptr, *d_log_bw = nullptr, *knot_sq = nullptr;
  int32_t *finish_inc = nullptr;
  // the delta head (stdadk_train_step_delta_f32): the derived output layer is rebuilt in front of the forward and the
  // head workgroup of the finishing launch folds its gradient into the delta rows (close_step fills sq_part / pending /
  // job); with fixed knots too the step then ends in that launch (finish_inc)
  const HeadFinishArgs *head = nullptr;
};
struct StepOut { const float *sq_parts = nullptr; int sq_n = 0; bool binned_next = false; };
struct NextBatch {   // the batch a one-call step announces (stdadk_train_step_next_f32)
  const int64_t *idx = nullptr;
  int64_t B = 0;
  int32_t y_cols = 0;
  void *workspace = nullptr;
  size_t workspace_bytes = 0;
  int32_t *binned = nullptr;   // set to 1 once the batch sits binned in `workspace`
};

static const StepRide NO_RIDE;

// The description of one opened call: written by the opener (open_mlp / open_step) and the door's own preamble (loss,
// targets, idx, auxiliary stream, fuse_tail, ride), then read-only -- every stage below takes it as `const Ctx &`.
// What one stage of a step produces for a later one travels by value between them, visible in their caller: the
// row-local launches the forward holds back (Held), the weight-gradient jobs behind the dZ launch (DwJobs), and what
// the step's closing launches left for the optimiser (StepOut).
struct Ctx {
  const stdadk_mlp_desc *d = nullptr;
  const stdadk_mlp_tensors *P = nullptr, *G = nullptr;
  float *ws = nullptr;
  Plan pl = {};
  hipStream_t st = nullptr;
  int64_t B = 0;
  const stdadk_basis_desc *basis = nullptr;   // step-level calls (open_step)
  bool window = false;          // the step runs the window path (want_window)
  bool w0t = false;             // W[0] / dW[0] stored (in,out)
  float dp = 0.f;               // effective dropout probability (0 in eval)
  uint64_t seed = 0;
  const int *step_dev = nullptr;
  const uint8_t *const *masks = nullptr;
  bool scattered = false;       // STDADK_FLAG_SCATTERED: the knots of a level sit anywhere (window path through knot cell lists)
  bool bf16 = false;            // STDADK_FLAG_BF16: bf16 operands in the fused tail kernels (P->W_bf16 / WT_bf16)
  bool pack = false;            // STDADK_FLAG_PACK_F32: fragment-order fp32 weight copies in the fused tail kernels (the
                                // P->W_bf16 / WT_bf16 slots read as float *PF / *PB)
  bool save = true;             // false in eval mode: the forward keeps nothing for a backward (xhat, rstd, act, psi)
  bool log_bw = false;          // basis->s_bw holds log-bandwidths (learnable knots)
  bool prebinned = false;       // window path: stdadk_bin_batch_f32 already filled the workspace's bins
  // ---- the door's preamble
  const int64_t *idx = nullptr; // window path: the batch is rows idx[b] of the resident observation arrays
  LossDev loss = LOSS_PLAIN_MSE;
  // fused loss (tail path): targets in the row order of the activations; outputs optional
  const float *mse_y = nullptr;
  float mse_scale = 0.f;
  float *mse_dY = nullptr;
  float *mse_loss = nullptr;
  bool fuse_tail = false;       // training step: the forward may hold its row-local launches back for the backward's
  // optional second stream: independent kernels of a step fork onto it (hipGraph-capturable
  // fork/join through events); NULL = everything on `st`
  hipStream_t aux = nullptr;
  const StepRide *ride = &NO_RIDE;   // what the one-call step lets ride along with its launches
};

// The row-local launches a training forward filled but did not issue: the backward's row-local launch runs them with
// the backward chain as ONE kernel (layer 0 of the window path, the tail forward and the loss are row-local, like the
// tail backward).  Caller-owned storage, filled in place.
struct Held {
  TailFwdArgs tail;
  L1FwdArgs l1;
  bool tail_held = false, l1_held = false;   // l1_held only with tail_held
  bool cap32 = false;           // this batch's tail launches use <= 32-row tiles (bf16 + dense layer 0 in the launch)
  bool loss_fused = false;      // the tail launch computes the loss (issued or held)
};

// materialising path, small D: layer 0 starts inside the tail launch from the raw observations (TailDense0)
struct Dense0Src { const float *coords, *t, *X, *s_bw; };

// an extra product C[M][H0] = A^T dZ_0 (reduction over the batch) to run with the dW GEMMs of the fused-tail
// backward: the temporal / covariate rows of dW0^T on the window path
struct ExtraProduct { const float *A; int64_t lda; int M; float *C; };

// What is left to do behind the dZ launch of the fused-tail backward: the dW products as one grouped launch, every
// fixed-order sum as one reductions launch.  Collected by collect_dw_jobs; its caller launches them or merges them
// into the per-knot gather.
struct DwJobs {
  GemmGroup gg;
  ReduceGroup rg;
  bool all_grouped = true;      // false: a product was not groupable and went out as a stand-alone GEMM
  bool dw0_in_group = false;    // materialising path: dW0^T joined the group
  bool head_apart = false;      // delta step: the output layer's two sums are head_job, not in rg -- the head workgroup
  ReduceJob head_job[2];        // of the finishing launch runs them (and their squares stay out of the clip norm)
};

// fork/join between the main and the auxiliary stream (events are created once per thread)
static hipEvent_t *fork_events() {
  static thread_local hipEvent_t ev[4];
  static thread_local bool made = false;
  if (!made) {
    for (int i = 0; i < 4; ++i)
      if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return nullptr;
    made = true;
  }
  return ev;
}
// `to` waits for everything enqueued on `from` so far
static int stream_depends(hipStream_t to, hipStream_t from, int slot) {
  if (g_dry_run) return 0;
  hipEvent_t *ev = fork_events();
  STDADK_REQUIRE(ev != nullptr, STDADK_E_ARG, "could not create fork/join events");
  hipError_t e = hipEventRecord(ev[slot], from);
  if (e == hipSuccess) e = hipStreamWaitEvent(to, ev[slot], 0);
  if (e != hipSuccess) { set_error("stream fork/join: %s", hipGetErrorString(e)); return (int)e; }
  return 0;
}

static bool tail_enabled() {
  static int v = -1;
  if (v < 0) {
    const char *e = getenv("STDADK_NO_FUSED_TAIL");
    v = (e && e[0] == '1') ? 0 : 1;
  }
  return v != 0;
}

// layer l of the model as the tail kernels take it: saving nothing (xhat, rstd, act NULL), or into the workspace of `c`
static TailLayer tail_layer(const stdadk_mlp_desc *d, const stdadk_mlp_tensors *P, bool bf16, int l, bool pack = false) {
  TailLayer t;
  t.W = P->W[l]; t.b = P->b[l];
  t.Wbf = bf16 ? P->W_bf16[l] : nullptr; t.WTbf = bf16 ? P->WT_bf16[l] : nullptr;
  t.PF = pack ? reinterpret_cast<const float *>(P->W_bf16[l]) : nullptr;
  t.PB = pack ? reinterpret_cast<const float *>(P->WT_bf16[l]) : nullptr;
  t.g = d->layernorm ? P->ln_g[l] : nullptr; t.be = d->layernorm ? P->ln_b[l] : nullptr;
  t.h = d->hidden[l]; t.hp = l > 0 ? d->hidden[l - 1] : d->in_dim;
  t.xhat = t.rstd = t.act = nullptr;
  t.layer_id = l;
  return t;
}
static TailLayer tail_layer(const Ctx &c, int l) {
  TailLayer t = tail_layer(c.d, c.P, c.bf16, l, c.pack);
  t.xhat = c.ws + c.pl.xhat[l]; t.rstd = c.ws + c.pl.rstd[l]; t.act = c.ws + c.pl.act[l];
  return t;
}
// what a tail forward launch takes from the model alone: output layer, Q, LayerNorm; no loss, the default objective
static void tail_fwd_model(TailFwdArgs &a, const stdadk_mlp_desc *d, const stdadk_mlp_tensors *P) {
  a.Wo = P->W[d->n_hidden]; a.bo = P->b[d->n_hidden]; a.Q = d->out_dim;
  a.layernorm = d->layernorm; a.eps = d->ln_eps;
  a.y = nullptr; a.grad_scale = 0.f; a.dY = nullptr; a.loss_sum = nullptr; a.loss = LOSS_PLAIN_MSE; a.loss.y_cols = a.Q;
}

// one hidden layer with the generic kernels: z = in W^T (+b) -> LN -> ReLU -> Dropout
static int generic_layer_forward(const Ctx &c, int l, const float *in, int64_t ld_in, int K) {
  const stdadk_mlp_desc *d = c.d;
  const stdadk_mlp_tensors *P = c.P;
  float *ws = c.ws;
  const Plan &pl = c.pl;
  const int64_t B = c.B;
  hipStream_t st = c.st;
  const int h = d->hidden[l];
  STDADK_REQUIRE(P->W[l] && P->b[l], STDADK_E_ARG, "mlp_forward: layer %d weights NULL", l);
  STDADK_REQUIRE(!d->layernorm || (P->ln_g[l] && P->ln_b[l]), STDADK_E_ARG, "mlp_forward: layer %d LN NULL", l);
  float *xh = ws + pl.xhat[l], *act = ws + pl.act[l];
  int splits = 1, rc;
  // z partials: slabs when split, else straight into the xhat buffer (normalised in place below)
  if (l == 0 && c.w0t)
    rc = gemm_run(in, ld_in, false, P->W[l], h, true, (int)B, h, K, nullptr, xh, h, ws + pl.slab, true, &splits, st);
  else
    rc = gemm_run(in, ld_in, false, P->W[l], K, false, (int)B, h, K, nullptr, xh, h, ws + pl.slab, true, &splits, st);
  if (rc) return rc;
  const float *zsrc = splits > 1 ? ws + pl.slab : xh;
  const uint8_t *mk = (c.masks && c.dp > 0.f) ? c.masks[l] : nullptr;
  dim3 grid((unsigned)ceil_div(B, ROW_T / 64));
#define FWD(LN_, CPL_)                                                                                   \
  STDADK_LAUNCH((ln_relu_fwd_kernel<LN_, CPL_>), grid, dim3(ROW_T), 0, st, zsrc, splits,                 \
                (int64_t)B * h, P->b[l], LN_ ? P->ln_g[l] : (const float *)nullptr,                      \
                LN_ ? P->ln_b[l] : (const float *)nullptr, d->ln_eps, B, h, xh, ws + pl.rstd[l],         \
                act, c.dp, c.seed, c.step_dev, l, mk)
  if (d->layernorm) { if (h <= 64) FWD(true, 1); else if (h <= 128) FWD(true, 2); else if (h <= 256) FWD(true, 4); else FWD(true, 16); }
  else { if (h <= 64) FWD(false, 1); else if (h <= 128) FWD(false, 2); else if (h <= 256) FWD(false, 4); else FWD(false, 16); }
#undef FWD
  STDADK_CHECK_LAUNCH("ln_relu_fwd");
  return 0;
}

// "The fused tail applies": every layer after the first, the output layer, the loss and their backward run in the
// tail kernels (masks, widths the tail refuses and STDADK_NO_FUSED_TAIL take the generic kernels)
static bool fused_tail(const stdadk_mlp_desc *d, const uint8_t *const *masks = nullptr) {
  return tail_enabled() && !masks && d->n_hidden >= 1 && tail_supported(d, 1);
}
static bool fused_tail(const Ctx &c) { return fused_tail(c.d, c.masks); }

// "Layer 0 runs inside the tail launch" (materialising path): small feature width, (in,out) first weight, fused tail
// available (environment STDADK_NO_DENSE0_TAIL=1: the separate kernels, diagnostic)
static bool dense0_in_tail(const Ctx &c) {
  return !c.window && c.w0t && c.d->in_dim <= TAIL_D0_MAX && fused_tail(c) && c.pl.ldf == ((c.d->in_dim + 31) & ~31) &&
         getenv("STDADK_NO_DENSE0_TAIL") == nullptr;
}

// where the backward leaves dZ of layer 0 (fused tail: its per-layer buffer; generic: the shared one)
static const float *layer0_dz(const Ctx &c) { return c.ws + (fused_tail(c) ? c.pl.dZl[0] : c.pl.dZ); }

// hidden layers [l0, L) and the output layer; `in` = input of layer l0 (`d0`: layer 0 inside the tail launch instead).
// When the fused tail applies, every layer after the first, the output layer and (if c.mse_y is set) the loss are ONE
// launch: its arguments are filled into `a` and *tail is set -- the caller issues it (tail_forward) or holds it for
// the backward's launch; what comes before it is issued here.  Otherwise the generic kernels are issued.
static int run_forward(const Ctx &c, int l0, const float *in, int64_t ld_in, int K, float *y_pred, const Dense0Src *d0,
                       TailFwdArgs &a, bool *tail) {
  const stdadk_mlp_desc *d = c.d;
  const stdadk_mlp_tensors *P = c.P;
  float *ws = c.ws;
  const Plan &pl = c.pl;
  const int64_t B = c.B;
  hipStream_t st = c.st;
  const int L = d->n_hidden, Q = d->out_dim;
  int rc;
  *tail = false;
  STDADK_REQUIRE(P->W[L] && P->b[L], STDADK_E_ARG, "mlp_forward: output layer weights NULL");
  if (fused_tail(c)) {
    int l = l0;
    a.d0.on = 0;
    if (l == 0 && d0) {
      // layer 0 inside the tail launch: features of a row tile in LDS, W0^T rows as the B operand
      static const float cals[3] = {1.000000f, 0.223477f, 0.654714f};  // st_interp.py:56-60
      const stdadk_basis_desc *b = c.basis;
      TailDense0 &z = a.d0;
      z.on = 1;
      z.coords = d0->coords; z.t = d0->t; z.X = d0->X;
      z.p = b->p; z.Ks = (int)b->Ks; z.Kt = (int)b->Kt; z.basis = b->basis; z.cal = cals[b->basis];
      z.s_centers = b->s_centers; z.s_bw = d0->s_bw; z.t_centers = b->t_centers; z.t_bw = b->t_bw;
      z.feats = c.save ? ws + pl.feats : nullptr; z.ldf = pl.ldf;
      z.W0T = P->W[0];
      z.L0 = tail_layer(c, 0);
      if (!c.save) z.L0.xhat = z.L0.rstd = z.L0.act = nullptr;
      l = 1;
    } else if (l == 0) {
      rc = generic_layer_forward(c, 0, in, ld_in, K);
      if (rc) return rc;
      l = 1;
    }
    a.n_layers = L - l;
    for (int i = l; i < L; ++i) {
      STDADK_REQUIRE(P->W[i] && P->b[i] && (!d->layernorm || (P->ln_g[i] && P->ln_b[i])), STDADK_E_ARG,
                     "mlp_forward: layer %d parameters NULL", i);
      a.L[i - l] = tail_layer(c, i);
      if (!c.save) a.L[i - l].xhat = a.L[i - l].rstd = a.L[i - l].act = nullptr;
    }
    a.a_in = ws + pl.act[l - 1];
    a.h_in = d->hidden[l - 1];
    a.B = (int)B;
    tail_fwd_model(a, d, P);
    a.y_pred = y_pred;
    a.y = c.mse_y; a.grad_scale = c.mse_scale; a.dY = c.mse_dY; a.loss_sum = c.mse_loss;
    a.loss = c.loss;
    if (a.loss.y_cols == 0) a.loss.y_cols = Q;
    a.drop_p = c.dp; a.seed = c.seed; a.step_dev = c.step_dev;
    a.bf16 = c.bf16 ? 1 : 0;
    { const char *e = getenv("STDADK_TAIL_STAMPS"); a.stamps = e ? (unsigned long long *)strtoull(e, nullptr, 0) : nullptr; }
    *tail = true;
    return 0;
  }
  for (int l = l0; l < L; ++l) {
    rc = generic_layer_forward(c, l, in, ld_in, K);
    if (rc) return rc;
    in = ws + pl.act[l]; ld_in = d->hidden[l]; K = d->hidden[l];
  }
  if (Q <= HEAD_MAXQ && ld_in == K) {
    STDADK_LAUNCH(head_fwd_kernel, dim3((unsigned)ceil_div(B, ROW_T / 64)), dim3(ROW_T), 0, st, in, B,
                  K, P->W[L], P->b[L], Q, y_pred);
    STDADK_CHECK_LAUNCH("head_fwd");
  } else {
    STDADK_REQUIRE(!(L == 0 && c.w0t), STDADK_E_ARG, "mlp_forward: transposed W0 needs a hidden layer");
    rc = gemm_run(in, ld_in, false, P->W[L], K, false, (int)B, Q, K, P->b[L], y_pred, Q, ws + pl.slab, false, nullptr, st);
    if (rc) return rc;
  }
  return 0;
}

// ---- the fused-tail backward: (a) the row-local launch, (b) collect the weight-gradient jobs, (c) launch them.
// Its callers write the composition out; between (a) and (b) dZ of every layer is final, so independent consumers
// (the per-knot gather on an auxiliary stream) may fork there, and a window-path step merges the jobs of (b) into the
// per-knot gather in place of (c) (close_step).

// (a) One kernel for the whole activation-gradient path -- with the launches the forward held back in front of it:
// tail_backward, tail_forward_backward or l1_tail_launch.  `fin` 2: the launch also clears the arrival counters of the
// merged weight-gradient launch.  *n_part: its workgroups = the rows of every column-sum partial it leaves.
static int tail_row_launch(const Ctx &c, const float *dY, bool layer0_dense, int fin, Held *h, int64_t *n_part) {
  const stdadk_mlp_desc *d = c.d;
  const stdadk_mlp_tensors *P = c.P, *G = c.G;
  float *ws = c.ws;
  const Plan &pl = c.pl;
  const int L = d->n_hidden;
  const bool held = h && h->tail_held;
  // (a split backward call cannot know whether its forward ran the dense layer 0 inside the launch: every
  //  bf16 backward on the materialising path with D <= TAIL_D0_MAX takes the 32-row cap the forward took)
  const bool cap32 = held ? h->cap32 : (c.bf16 && layer0_dense && c.w0t && d->in_dim <= TAIL_D0_MAX);
  *n_part = ceil_div(c.B, tail_rows(c.B, cap32));
  TailBwdArgs a;
  a.n_layers = L;
  for (int l = 0; l < L; ++l) {
    STDADK_REQUIRE(G->W[l] && G->b[l] && (!d->layernorm || (G->ln_g[l] && G->ln_b[l])), STDADK_E_ARG,
                   "mlp_backward: layer %d grads NULL", l);
    a.L[l] = tail_layer(c, l);
    a.dZ[l] = ws + pl.dZl[l];
    a.part[l] = ws + pl.partl[l];
  }
  STDADK_REQUIRE(G->W[L] && G->b[L], STDADK_E_ARG, "mlp_backward: output layer grads NULL");
  a.B = (int)c.B; a.Wo = P->W[L]; a.Q = d->out_dim; a.dY = dY;
  a.act_last = ws + pl.act[L - 1]; a.part_head = ws + pl.part;
  a.layernorm = d->layernorm; a.drop_p = c.dp; a.seed = c.seed; a.step_dev = c.step_dev;
  a.bf16 = c.bf16 ? 1 : 0;
  a.zero_ints = fin == 2 ? reinterpret_cast<int *>(ws + pl.fin_cnt) : nullptr;
  a.n_zero = fin == 2 ? FIN_TILES_MAX : 0;
  { const char *e = getenv("STDADK_TAIL_BWD_STAMPS"); a.stamps = e ? (unsigned long long *)strtoull(e, nullptr, 0) : nullptr; }
  if (!held) return tail_backward(a, c.st, cap32);
  h->tail_held = false;
  if (!h->l1_held) return tail_forward_backward(h->tail, a, c.st);
  h->l1_held = false;
  return l1_tail_launch(h->l1, c.basis->basis, d->layernorm != 0, h->tail, a, c.st);
}

// (b) ONE grouped launch for the dW products, ONE grouped launch for every fixed-order sum: collects them into `j` and
// launches nothing -- except a product that cannot join the group, which goes out as a stand-alone GEMM right here.
// `extra`: products with dZ_0 that ride along; `features` (materialising path, else NULL): dW0^T joins while it is a
// split-K product; `fin` 2: the slabs of the products are summed by the merged launch itself, not by a reduce job.
// `head_apart` (delta step): the output layer's two sums go to j.head_job, not into the table.
static int collect_dw_jobs(const Ctx &c, int64_t n_part, int fin, const ExtraProduct *extra, int n_extra,
                           const float *features, int64_t ldf, DwJobs &j, bool head_apart = false) {
  const stdadk_mlp_desc *d = c.d;
  const stdadk_mlp_tensors *G = c.G;
  float *ws = c.ws;
  const Plan &pl = c.pl;
  const int64_t B = c.B;
  const int L = d->n_hidden, Q = d->out_dim, hL = d->hidden[L - 1];
  float *part = ws + pl.part, *slab = ws + pl.slab;
  const float *dz0 = ws + pl.dZl[0];
  GemmGroup &gg = j.gg;
  ReduceGroup &rg = j.rg;
  size_t slab_off = 0;
  int rc;
  auto add_reduce = [&](const float *src, float *dst, int n, int splits, int64_t stride) -> bool {
    if (rg.n >= REDUCE_GROUP_MAX) return false;
    ReduceJob &r = rg.job[rg.n++];
    r.src = src; r.dst = dst; r.n = n; r.splits = splits; r.stride = stride;
    return true;
  };
  // C[M][N] (contiguous) = A^T Bm, both operands stored [B rows][.]; falls back to a stand-alone GEMM
  // (`bf`: a layer after the first under STDADK_FLAG_BF16 -- operands rounded to bf16 at the LDS boundary)
  auto add_tn = [&](const float *A, int64_t lda, const float *Bm, int64_t ldb, int M, int N, float *C,
                    bool bf = false) -> int {
    if (gg.n < GEMM_GROUP_MAX && rg.n < REDUCE_GROUP_MAX && gemm_tn_groupable(A, lda, Bm, ldb)) {
      GemmArgs &g = gg.job[gg.n++];
      g.A = A; g.lda = lda; g.B = Bm; g.ldb = ldb; g.C = C; g.ldc = N; g.bias = nullptr;
      g.M = M; g.N = N; g.K = (int)B;
      g.bf16 = bf ? 1 : 0;
      g.splits = gemm_pick_splits(M, N, (int)B, &g.kps, false);
      g.slab = slab + slab_off; g.slab_stride = (int64_t)M * N;
      slab_off += (size_t)g.splits * M * N;
      if (fin != 2) add_reduce(g.slab, C, M * N, g.splits, g.slab_stride);   // 2: the last K slice to arrive sums
      return 0;
    }
    j.all_grouped = false;
    return gemm_run(A, lda, true, Bm, ldb, true, M, N, (int)B, nullptr, C, N, slab + slab_off, false, nullptr, c.st);
  };
  if (head_apart) {
    j.head_apart = true;
    j.head_job[0] = ReduceJob{part, G->W[L], Q * hL, (int)n_part, (int64_t)Q * (hL + 1)};
    j.head_job[1] = ReduceJob{part + Q * hL, G->b[L], Q, (int)n_part, (int64_t)Q * (hL + 1)};
  } else {
    add_reduce(part, G->W[L], Q * hL, (int)n_part, (int64_t)Q * (hL + 1));
    add_reduce(part + Q * hL, G->b[L], Q, (int)n_part, (int64_t)Q * (hL + 1));
  }
  for (int l = L - 1; l >= 0; --l) {
    const int h = d->hidden[l];
    const float *pp = ws + pl.partl[l];
    if (d->layernorm) {
      add_reduce(pp, G->ln_g[l], h, (int)n_part, (int64_t)3 * h);
      add_reduce(pp + h, G->ln_b[l], h, (int)n_part, (int64_t)3 * h);
    }
    add_reduce(pp + 2 * h, G->b[l], h, (int)n_part, (int64_t)3 * h);
    if (l == 0) break;
    // dW_l[h][kin] = dZ_l^T act_{l-1}
    rc = add_tn(ws + pl.dZl[l], h, ws + pl.act[l - 1], d->hidden[l - 1], h, d->hidden[l - 1], G->W[l], c.bf16);
    if (rc) return rc;
  }
  for (int e = 0; e < n_extra; ++e) {
    rc = add_tn(extra[e].A, extra[e].lda, dz0, d->hidden[0], extra[e].M, d->hidden[0], extra[e].C);
    if (rc) return rc;
  }
  if (features && c.w0t) {
    // materialising path with the (in,out) layout: while dW0^T = features^T dZ_0 is a split-K product
    // (few tiles: small D) it joins the grouped launch and its slabs the grouped reduction -- two launches
    // fewer than a stand-alone GEMM + slab sum; a D that fills the chip on its own keeps its direct GEMM
    int kps;
    const int h0 = d->hidden[0];
    const int sp = gemm_pick_splits(d->in_dim, h0, (int)B, &kps, false);
    if (sp > 1 && slab_off + (size_t)sp * d->in_dim * h0 <= pl.slab_floats) {
      rc = add_tn(features, ldf, dz0, h0, d->in_dim, h0, G->W[0]);
      if (rc) return rc;
      j.dw0_in_group = true;
    }
  }
  return 0;
}

// (c) the two grouped launches; materialising path (`features`): then dW0 as a stand-alone GEMM unless it joined the group
// (`reduce` false: the reductions are left to the caller's finishing launch)
static int launch_dw_jobs(const Ctx &c, DwJobs &j, const float *features, int64_t ldf, bool reduce = true) {
  int rc = launch_gemm_tn_grouped(j.gg, c.st);
  if (rc) return rc;
  if (reduce) rc = launch_reduce_jobs(j.rg, c.st);
  if (rc || !features || j.dw0_in_group) return rc;
  const stdadk_mlp_desc *d = c.d;
  const int h = d->hidden[0];
  const float *dz0 = c.ws + c.pl.dZl[0];
  float *slab = c.ws + c.pl.slab;
  if (c.w0t)
    return gemm_run(features, ldf, true, dz0, h, true, d->in_dim, h, (int)c.B, nullptr, c.G->W[0], h, slab, false, nullptr, c.st);
  return gemm_run(dz0, h, true, features, ldf, true, h, d->in_dim, (int)c.B, nullptr, c.G->W[0], d->in_dim, slab, false, nullptr, c.st);
}

// The backward with the generic kernels (masks, widths the tail refuses, STDADK_NO_FUSED_TAIL): output layer, then
// hidden layers L-1 .. 0.  With `layer0_dense` false the first layer stops after dZ_0 and its bias / LayerNorm
// gradients (dW0 is produced by the window kernels).
static int generic_backward(const Ctx &c, const float *dY, const float *features, int64_t ldf, bool layer0_dense) {
  const stdadk_mlp_desc *d = c.d;
  const stdadk_mlp_tensors *P = c.P, *G = c.G;
  float *ws = c.ws;
  const Plan &pl = c.pl;
  const int64_t B = c.B;
  hipStream_t st = c.st;
  const int L = d->n_hidden, Q = d->out_dim;
  const int rows = bwd_rows(B);
  const int64_t nblk = ceil_div(B, rows);
  float *dA = ws + pl.dA, *dZ = ws + pl.dZ, *part = ws + pl.part, *slab = ws + pl.slab;
  int rc;
  const float *aL = L > 0 ? ws + pl.act[L - 1] : features;
  const int64_t ldaL = L > 0 ? d->hidden[L - 1] : ldf;
  const int hL = L > 0 ? d->hidden[L - 1] : d->in_dim;
  STDADK_REQUIRE(G->W[L] && G->b[L], STDADK_E_ARG, "mlp_backward: output layer grads NULL");
  if (Q <= HEAD_MAXQ && L > 0) {
    STDADK_LAUNCH(head_bwd_kernel, dim3((unsigned)nblk), dim3(ROW_T), sizeof(float) * rows * Q, st, aL, dY,
                       B, hL, P->W[L], Q, dA, part, rows);
    STDADK_CHECK_LAUNCH("head_bwd");
    int n = Q * (hL + 1);
    STDADK_LAUNCH(head_reduce_kernel, dim3((unsigned)ceil_div(n, 64)), dim3(64 * CS_G), 0, st, part, nblk, Q, hL,
                       G->W[L], G->b[L]);
    STDADK_CHECK_LAUNCH("head_reduce");
  } else {
    // dW_out[Q][hL] = dY^T a ; db = colsum(dY) ; dA = dY W_out
    rc = gemm_run(dY, Q, true, aL, ldaL, true, Q, hL, (int)B, nullptr, G->W[L], hL, slab, false, nullptr, st);
    if (rc) return rc;
    ColsumOut co; co.o[0] = G->b[L]; co.o[1] = co.o[2] = nullptr;
    STDADK_LAUNCH(colsum_kernel, dim3((unsigned)ceil_div(Q, 64)), dim3(64 * CS_G), 0, st, dY, B, (int64_t)Q, Q, 1, co);
    STDADK_CHECK_LAUNCH("colsum");
    if (L > 0) {
      rc = gemm_run(dY, Q, false, P->W[L], hL, true, (int)B, hL, Q, nullptr, dA, hL, slab, false, nullptr, st);
      if (rc) return rc;
    }
  }

  for (int l = L - 1; l >= 0; --l) {
    const int h = d->hidden[l];
    const uint8_t *mk = (c.masks && c.dp > 0.f) ? c.masks[l] : nullptr;
    STDADK_REQUIRE(G->W[l] && G->b[l], STDADK_E_ARG, "mlp_backward: layer %d grads NULL", l);
#define BWD(LN_, CPL_)                                                                                   \
  STDADK_LAUNCH((ln_relu_bwd_kernel<LN_, CPL_>), dim3((unsigned)nblk), dim3(ROW_T), 0, st, dA,      \
                     ws + pl.xhat[l], ws + pl.rstd[l], LN_ ? P->ln_g[l] : (const float *)nullptr,        \
                     LN_ ? P->ln_b[l] : (const float *)nullptr, B, h, dZ, part, c.dp, c.seed,            \
                     c.step_dev, l, mk, rows)
    if (d->layernorm) { if (h <= 64) BWD(true, 1); else if (h <= 128) BWD(true, 2); else if (h <= 256) BWD(true, 4); else BWD(true, 16); }
    else { if (h <= 64) BWD(false, 1); else if (h <= 128) BWD(false, 2); else if (h <= 256) BWD(false, 4); else BWD(false, 16); }
#undef BWD
    STDADK_CHECK_LAUNCH("ln_relu_bwd");
    ColsumOut co;
    if (d->layernorm) {
      STDADK_REQUIRE(G->ln_g[l] && G->ln_b[l], STDADK_E_ARG, "mlp_backward: layer %d LN grads NULL", l);
      co.o[0] = G->ln_g[l]; co.o[1] = G->ln_b[l]; co.o[2] = G->b[l];
      STDADK_LAUNCH(colsum_kernel, dim3((unsigned)ceil_div(3 * h, 64)), dim3(64 * CS_G), 0, st, part, nblk,
                         (int64_t)3 * h, h, 3, co);
    } else {
      co.o[0] = G->b[l]; co.o[1] = co.o[2] = nullptr;
      STDADK_LAUNCH(colsum_kernel, dim3((unsigned)ceil_div(h, 64)), dim3(64 * CS_G), 0, st, part + 2 * h, nblk,
                         (int64_t)3 * h, h, 1, co);
    }
    STDADK_CHECK_LAUNCH("colsum");
    if (l == 0 && !layer0_dense) break;
    const float *ain = l > 0 ? ws + pl.act[l - 1] : features;
    const int64_t ldin = l > 0 ? d->hidden[l - 1] : ldf;
    const int kin = l > 0 ? d->hidden[l - 1] : d->in_dim;
    if (l == 0 && c.w0t)   // dW0^T[kin][h] = ain^T dZ
      rc = gemm_run(ain, ldin, true, dZ, h, true, kin, h, (int)B, nullptr, G->W[l], h, slab, false, nullptr, st);
    else                   // dW[h][kin] = dZ^T ain   (reduction over the batch)
      rc = gemm_run(dZ, h, true, ain, ldin, true, h, kin, (int)B, nullptr, G->W[l], kin, slab, false, nullptr, st);
    if (rc) return rc;
    if (l > 0) {
      // dA_prev[B][kin] = dZ W   (W stored [h][kin] => K-major B operand)
      rc = gemm_run(dZ, h, false, P->W[l], kin, true, (int)B, kin, h, nullptr, dA, kin, slab, false, nullptr, st);
      if (rc) return rc;
    }
  }
  return 0;
}

static int launch_mse(const float *yp, const float *y, int64_t n, float scale, float *dY, float *loss_sum,
                      hipStream_t st) {
  int64_t blocks = ceil_div(n, 256);
  if (blocks > 1024) blocks = 1024;
  STDADK_LAUNCH(mse_kernel, dim3((unsigned)blocks), dim3(256), 0, st, yp, y, n, scale, dY, loss_sum);
  STDADK_CHECK_LAUNCH("mse");
  return 0;
}

static int check_basis(const stdadk_basis_desc *b, const stdadk_mlp_desc *d) {
  STDADK_REQUIRE(b != nullptr, STDADK_E_ARG, "basis desc is NULL");
  STDADK_REQUIRE(b->p >= 0 && b->Ks >= 0 && b->Kt >= 0 && b->basis >= 0 && b->basis <= 2, STDADK_E_ARG,
                 "basis desc: bad sizes / kind");
  STDADK_REQUIRE(b->p + b->Ks + b->Kt == d->in_dim, STDADK_E_SHAPE, "basis desc: p+Ks+Kt=%lld != in_dim=%d",
                 (long long)(b->p + b->Ks + b->Kt), d->in_dim);
  STDADK_REQUIRE(b->Ks == 0 || (b->s_centers && b->s_bw), STDADK_E_ARG, "basis desc: spatial knots NULL");
  STDADK_REQUIRE(b->Kt == 0 || (b->t_centers && b->t_bw), STDADK_E_ARG, "basis desc: temporal knots NULL");
  if (b->n_levels > 0) {
    STDADK_REQUIRE(b->n_levels <= STDADK_MAX_LEVELS, STDADK_E_ARG, "basis desc: too many levels");
    int64_t k = 0, kc = 0;
    for (int l = 0; l < b->n_levels; ++l) {
      STDADK_REQUIRE(b->side[l] >= 1, STDADK_E_ARG, "basis desc: side[%d] < 1", l);
      k += (int64_t)b->side[l] * b->side[l];
      kc += b->side[l];
    }
    // uniform grid: side lengths; STDADK_FLAG_SCATTERED: level sizes (the flag is checked by the callers)
    STDADK_REQUIRE(k == b->Ks || kc == b->Ks, STDADK_E_SHAPE,
                   "basis desc: neither sum(side^2)=%lld nor sum(side)=%lld equals Ks=%lld", (long long)k, (long long)kc,
                   (long long)b->Ks);
  }
  return 0;
}

static inline bool is_scattered(const stdadk_basis_desc *b, int flags) {
  return (flags & STDADK_FLAG_SCATTERED) != 0 && b->n_levels > 0;
}
static int check_levels(const stdadk_basis_desc *b, int flags) {
  if (b->n_levels <= 0) return 0;
  int64_t k = 0;
  for (int l = 0; l < b->n_levels; ++l) k += is_scattered(b, flags) ? (int64_t)b->side[l] : (int64_t)b->side[l] * b->side[l];
  STDADK_REQUIRE(k == b->Ks, STDADK_E_SHAPE, "basis desc: the level sizes add up to %lld, Ks = %lld%s", (long long)k,
                 (long long)b->Ks, is_scattered(b, flags) ? " (STDADK_FLAG_SCATTERED: side[] holds knot counts)" : "");
  return 0;
}

static inline int64_t learn_ks(const stdadk_basis_desc *b, int flags) {
  return (flags & STDADK_FLAG_LOG_BW) ? b->Ks : 0;
}

static bool want_window(const stdadk_basis_desc *b, const stdadk_mlp_desc *d, int flags) {
  if (flags & STDADK_FLAG_DENSE) return false;
  if (!(flags & STDADK_FLAG_W0_T)) return false;
  if (d->n_hidden < 1 || b->Ks <= 0 || b->Kt <= 0) return false;
  // small tables: materialising is cheap (D small) and the window path's per-knot gather is serial over
  // the many rows each coarse knot sees (MI355X, B = 4096, 227 knots: 0.34 ms window vs 0.15 ms dense)
  if (!(flags & STDADK_FLAG_WINDOW) && b->Ks < 1024) return false;
  if (is_scattered(b, flags) && b->n_levels > STDADK_MAX_LEVELS) return false;
  return l1_window_supported(b->n_levels, b->basis, d->hidden[0], b->p, (int)b->Kt);
}

static GridView make_grid(const stdadk_basis_desc *b, bool scattered = false) {
  static const float cals[3] = {1.000000f, 0.223477f, 0.654714f};   // st_interp.py:56-60
  GridView g;
  g.n_levels = b->n_levels;
  g.scattered = scattered ? 1 : 0;
  int off = 0;
  for (int l = 0; l < STDADK_MAX_LEVELS; ++l) {
    const int v = l < b->n_levels ? b->side[l] : 0;
    g.side[l] = scattered ? 0 : v;
    g.cnt[l] = scattered ? v : v * v;
    g.off[l] = off;
    off += g.cnt[l];
  }
  g.p = b->p; g.Ks = (int)b->Ks; g.Kt = (int)b->Kt;
  g.cal = cals[b->basis];
  g.centers = b->s_centers; g.bw = b->s_bw; g.t_centers = b->t_centers; g.t_bw = b->t_bw;
  return g;
}

static BinBuffers plan_bins(float *ws, const Plan &pl) {
  BinBuffers bb;
  bb.keys = (int *)(ws + pl.keys); bb.hist = (int *)(ws + pl.hist); bb.cursor = (int *)(ws + pl.cursor);
  bb.cell_start = (int *)(ws + pl.cell_start); bb.perm_tmp = (int *)(ws + pl.perm_tmp);
  bb.perm = (int *)(ws + pl.perm);
  bb.xs = ws + pl.xs; bb.ys = ws + pl.ys; bb.ts = ws + pl.ts; bb.y_s = ws + pl.y_s; bb.X_s = ws + pl.X_s;
  return bb;
}

// scattered knots: bin the knots of every level into cells (knot_bins) and point the forward at the lists
static int scattered_bins(const Ctx &c, L1FwdArgs &a) {
  const Plan &pl = c.pl;
  const stdadk_basis_desc *b = c.basis;
  int *kcs = (int *)(c.ws + pl.kcs), *kperm = (int *)(c.ws + pl.kperm), *ktmp = (int *)(c.ws + pl.kperm_tmp);
  float *reach = c.ws + pl.reach;
  int rc;
  if (c.log_bw) {
    a.g.bw = c.ws + pl.bw_exp;
    rc = knot_bins(a.g, kcs, kperm, ktmp, reach, c.st, b->s_bw, c.ws + pl.bw_exp);
  } else {
    rc = knot_bins(a.g, kcs, kperm, ktmp, reach, c.st);
  }
  if (rc) return rc;
  a.kcs = kcs; a.kperm = kperm; a.reach = reach; a.Gk = KNOT_CELLS;
  return 0;
}

// Window path, in front of layer 0: bins the batch (and the knots, where they move) and fills the arguments of the
// feature build + layer 0 launch (sorted order) into `a`; the caller issues it (l1_window_forward) or holds it
static int window_layer0_forward(const Ctx &c, const float *coords, const float *t, const float *X, const float *y,
                                 L1FwdArgs &a) {
  const Plan &pl = c.pl;
  const stdadk_basis_desc *b = c.basis;
  BinBuffers bb = plan_bins(c.ws, pl);
  int rc = 0;
  if (!c.prebinned) {
    STDADK_REQUIRE(coords && t && (b->p == 0 || X), STDADK_E_ARG, "step: NULL observation pointer");
    rc = bin_obs(coords, t, y, c.loss.y_cols ? c.loss.y_cols : c.d->out_dim, X, b->p, (int)c.B, pl.G, bb, c.st,
                 c.idx);
    if (rc) return rc;
  }
  a.g = make_grid(b, c.scattered);
  a.halo = nullptr;
  if (c.scattered) {
    // knots anywhere: this step's cell lists of the knots (and exp(log_bw) for learnable ones)
    rc = scattered_bins(c, a);
    if (rc) return rc;
  } else if (c.log_bw) {
    // learnable knots: bandwidth = exp(log_bandwidth) (st_interp.py:146-148), and the candidate
    // windows follow wherever the knots are now
    a.g.bw = c.ws + pl.bw_exp;
    rc = knot_halo(a.g, c.ws + pl.halo, c.st, b->s_bw, c.ws + pl.bw_exp);   // also fills bw_exp
    if (rc) return rc;
    a.halo = c.ws + pl.halo;
  }
  a.xs = bb.xs; a.ys = bb.ys; a.ts = bb.ts; a.Xs = b->p > 0 ? bb.X_s : nullptr;
  a.B = (int)c.B; a.H = c.d->hidden[0];
  a.W0T = c.P->W[0]; a.b0 = c.P->b[0];
  a.gamma = c.d->layernorm ? c.P->ln_g[0] : nullptr;
  a.beta = c.d->layernorm ? c.P->ln_b[0] : nullptr;
  a.eps = c.d->ln_eps;
  a.xhat = c.ws + pl.xhat[0]; a.rstd = c.ws + pl.rstd[0]; a.act = c.ws + pl.act[0];
  a.psi = c.ws + pl.psi; a.ld_psi = pl.ld_psi;
  if (!c.save) a.xhat = a.rstd = a.psi = nullptr;      // act stays: it is the input of the next layer
  a.drop_p = c.dp; a.seed = c.seed; a.step_dev = c.step_dev;
  a.rows_per_wg = 0; a.n_wg = 0;
  STDADK_REQUIRE(a.W0T && a.b0, STDADK_E_ARG, "window forward: layer 0 weights NULL");
  return 0;
}

// The opener of the two stdadk_mlp_*_f32 doors: plans and fills `c`; false = workspace too small (worded by the door)
static bool open_mlp(Ctx &c, const stdadk_mlp_desc *d, int64_t B, void *workspace, size_t workspace_bytes,
                     const stdadk_mlp_tensors *P, const stdadk_mlp_tensors *G, stdadk_stream_t stream, bool training,
                     uint64_t drop_seed, const uint8_t *const *drop_mask) {
  make_plan(d, B, &c.pl);
  if (workspace_bytes < c.pl.total_floats * sizeof(float)) return false;
  c.d = d; c.P = P; c.G = G; c.ws = (float *)workspace; c.st = (hipStream_t)stream; c.B = B;
  c.dp = training ? d->dropout_p : 0.f; c.seed = drop_seed; c.masks = drop_mask;
  return true;
}

}  // namespace stdadk

using namespace stdadk;

extern "C" size_t stdadk_mlp_workspace_bytes(const stdadk_mlp_desc *desc, int64_t B) {
  // (a batch beyond the 32-bit row indices of the kernels is refused here too: the planner casts B to int, and the
  //  host-side sanitizer pass found the division by zero a truncated 2^40 ran into)
  if (check_desc(desc) != 0 || B < 0 || B >= (1ll << 31)) return 0;
  Plan p;
  make_plan(desc, B > 0 ? B : 1, &p);
  return p.total_floats * sizeof(float);
}

extern "C" int stdadk_mlp_forward_f32(const stdadk_mlp_desc *d, const stdadk_mlp_tensors *P,
                                      const float *features, int64_t ldf, int64_t B, float *y_pred,
                                      void *workspace, size_t workspace_bytes, int32_t training,
                                      uint64_t drop_seed, const uint8_t *const *drop_mask,
                                      stdadk_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  STDADK_REQUIRE(B >= 0 && B < (1ll << 31), STDADK_E_ARG, "mlp_forward: bad B");
  if (B == 0) return 0;
  STDADK_REQUIRE(P && features && y_pred && workspace, STDADK_E_ARG, "mlp_forward: NULL pointer");
  STDADK_REQUIRE(ldf >= d->in_dim, STDADK_E_SHAPE, "mlp_forward: ldf %lld < in_dim %d", (long long)ldf, d->in_dim);
  STDADK_REQUIRE(aligned16(workspace), STDADK_E_ALIGN, "mlp_forward: workspace must be 16-byte aligned");
  Ctx c;
  STDADK_REQUIRE(open_mlp(c, d, B, workspace, workspace_bytes, P, nullptr, stream, training != 0, drop_seed, drop_mask),
                 STDADK_E_WORKSPACE, "mlp_forward: workspace %zu < %zu bytes", workspace_bytes,
                 c.pl.total_floats * sizeof(float));
  TailFwdArgs tail;
  bool is_tail;
  rc = run_forward(c, 0, features, ldf, d->in_dim, y_pred, nullptr, tail, &is_tail);
  if (rc || !is_tail) return rc;
  return tail_forward(tail, c.st);
}

extern "C" int stdadk_mlp_backward_f32(const stdadk_mlp_desc *d, const stdadk_mlp_tensors *P,
                                       const stdadk_mlp_tensors *G, const float *features,
                                       int64_t ldf, int64_t B, const float *dY, void *workspace,
                                       size_t workspace_bytes, uint64_t drop_seed,
                                       const uint8_t *const *drop_mask, stdadk_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  STDADK_REQUIRE(B > 0 && B < (1ll << 31), STDADK_E_ARG, "mlp_backward: bad B");
  STDADK_REQUIRE(P && G && features && dY && workspace, STDADK_E_ARG, "mlp_backward: NULL pointer");
  STDADK_REQUIRE(ldf >= d->in_dim, STDADK_E_SHAPE, "mlp_backward: ldf < in_dim");
  Ctx c;
  STDADK_REQUIRE(open_mlp(c, d, B, workspace, workspace_bytes, P, G, stream, true, drop_seed, drop_mask),
                 STDADK_E_WORKSPACE, "mlp_backward: workspace too small");
  if (!fused_tail(c)) return generic_backward(c, dY, features, ldf, true);
  int64_t n_part;
  DwJobs jobs;
  rc = tail_row_launch(c, dY, true, 0, nullptr, &n_part);
  if (rc) return rc;
  rc = collect_dw_jobs(c, n_part, 0, nullptr, 0, features, ldf, jobs);
  if (rc) return rc;
  return launch_dw_jobs(c, jobs, features, ldf);
}

extern "C" int stdadk_mse_f32(const float *y_pred, const float *y, int64_t n, float grad_scale,
                              float *dY, float *loss_sum, stdadk_stream_t stream) {
  STDADK_REQUIRE(n >= 0, STDADK_E_ARG, "mse: negative n");
  if (n == 0) return 0;
  STDADK_REQUIRE(y_pred && y, STDADK_E_ARG, "mse: NULL pointer");
  return launch_mse(y_pred, y, n, grad_scale, dY, loss_sum, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// step-level entry points: observations in, predictions / gradients out
// ---------------------------------------------------------------------------------------------
extern "C" int32_t stdadk_step_uses_window(const stdadk_basis_desc *b, const stdadk_mlp_desc *d, int32_t flags) {
  if (check_desc(d) != 0 || check_basis(b, d) != 0) return 0;
  return want_window(b, d, flags) ? 1 : 0;
}

// the workspace plan of a step on `B` rows (the scattered-knot buffers exist on the window path only)
static void plan_step(const stdadk_basis_desc *b, const stdadk_mlp_desc *d, int64_t B, int32_t flags, Plan *p) {
  make_plan(d, B, p, want_window(b, d, flags) ? PLAN_STEP_WINDOW : PLAN_STEP_DENSE, b->p, (int)b->Kt, learn_ks(b, flags),
            is_scattered(b, flags) ? b->Ks : 0, b->n_levels, b->Ks);
}

extern "C" size_t stdadk_step_workspace_bytes(const stdadk_basis_desc *b, const stdadk_mlp_desc *d, int64_t B,
                                              int32_t flags) {
  if (check_desc(d) != 0 || check_basis(b, d) != 0 || B < 0 || B >= (1ll << 31)) return 0;
  Plan p;
  plan_step(b, d, B > 0 ? B : 1, flags, &p);
  return p.total_floats * sizeof(float);
}

// The one opener of a step-level Ctx: validates descriptors, batch size, workspace and flags, plans, fills `c` (`training`
// false: no dropout, nothing kept for a backward).  P and G are stored unchecked: each door refuses NULLs in its own words.
static int open_step(Ctx &c, const stdadk_basis_desc *b, const stdadk_mlp_desc *d, int64_t B, void *workspace,
                     size_t workspace_bytes, int32_t flags, const stdadk_mlp_tensors *P,
                     const stdadk_mlp_tensors *G, stdadk_stream_t stream, bool training, uint64_t drop_seed = 0,
                     const int32_t *step_dev = nullptr) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_basis(b, d);
  if (rc) return rc;
  STDADK_REQUIRE(B > 0 && B < (1ll << 31), STDADK_E_ARG, "step: bad B");
  STDADK_REQUIRE(workspace && aligned16(workspace), STDADK_E_ALIGN, "step: workspace NULL or not 16-byte aligned");
  c.window = want_window(b, d, flags);
  rc = check_levels(b, flags);
  if (rc) return rc;
  c.scattered = c.window && is_scattered(b, flags);
  plan_step(b, d, B, flags, &c.pl);
  c.log_bw = (flags & STDADK_FLAG_LOG_BW) != 0;
  c.bf16 = (flags & STDADK_FLAG_BF16) != 0;
  STDADK_REQUIRE(!c.bf16 || fused_tail(d), STDADK_E_ARG,
                 "step: STDADK_FLAG_BF16 needs the fused tail kernels (hidden widths multiples of 16 up to %d, out_dim <= %d)",
                 TAIL_MAX_W, TAIL_MAXQ);
  c.pack = (flags & STDADK_FLAG_PACK_F32) != 0;
  if (c.pack) {
    STDADK_REQUIRE(!c.bf16, STDADK_E_ARG, "step: STDADK_FLAG_PACK_F32 and STDADK_FLAG_BF16 exclude each other");
    STDADK_REQUIRE(fused_tail(d), STDADK_E_ARG,
                   "step: STDADK_FLAG_PACK_F32 needs the fused tail kernels (hidden widths multiples of 16 up to %d, "
                   "out_dim <= %d)", TAIL_MAX_W, TAIL_MAXQ);
    for (int l = 1; P && l < d->n_hidden; ++l) {
      STDADK_REQUIRE(P->W_bf16[l] && P->WT_bf16[l], STDADK_E_ARG,
                     "step: STDADK_FLAG_PACK_F32 needs the packed copies of layer %d (params->W_bf16 / WT_bf16 as "
                     "float *; stdadk_f32_pack_refresh)", l);
      STDADK_REQUIRE(aligned16(P->W_bf16[l]) && aligned16(P->WT_bf16[l]), STDADK_E_ALIGN,
                     "step: the packed copies of layer %d must be 16-byte aligned", l);
    }
  }
  STDADK_REQUIRE(workspace_bytes >= c.pl.total_floats * sizeof(float), STDADK_E_WORKSPACE,
                 "step: workspace %zu < %zu bytes", workspace_bytes, c.pl.total_floats * sizeof(float));
  c.d = d; c.P = P; c.G = G; c.ws = (float *)workspace; c.st = (hipStream_t)stream; c.B = B;
  c.basis = b; c.w0t = (flags & STDADK_FLAG_W0_T) != 0;
  c.dp = training ? d->dropout_p : 0.f; c.seed = drop_seed; c.step_dev = step_dev; c.save = training;
  c.prebinned = c.window && (flags & STDADK_FLAG_PREBINNED) != 0;
  STDADK_REQUIRE(c.window || !(flags & STDADK_FLAG_PREBINNED), STDADK_E_ARG,
                 "step: STDADK_FLAG_PREBINNED needs the window path");
  return 0;
}

// dW0^T spatial rows (window path): every knot row by the wave that owns it
static L1BwdArgs window_gather_args(const Ctx &c) {
  float *ws = c.ws;
  L1BwdArgs a;
  a.g = make_grid(c.basis, c.scattered);
  a.xs = ws + c.pl.xs; a.ys = ws + c.pl.ys;
  a.cell_start = (const int *)(ws + c.pl.cell_start);
  a.G = c.pl.G; a.B = (int)c.B; a.H = c.d->hidden[0];
  a.dZ = layer0_dz(c); a.dW0T = c.G->W[0];
  a.W0T = nullptr; a.kpart = nullptr;
  if (c.log_bw) {      // learnable knots: the same pass also yields the raw knot gradients
    a.g.bw = ws + c.pl.bw_exp;
    a.W0T = c.P->W[0];
    a.kpart = ws + c.pl.kpart;
  }
  return a;
}
// ... as a launch of its own
static int window_gather(const Ctx &c, hipStream_t st) { return l1_window_backward(window_gather_args(c), c.basis->basis, st); }
// ... merged with the grouped dW products of `j` (dw_all.hip), which also bins the announced next batch; `fin`: with
// finishing work (FinArgs) -- the squared-norm slots, *n_slots of them out of `slot_cap`, and with fin->cnt the sums of
// `j.rg` as well
static int window_dw_all(const Ctx &c, DwJobs &j, const FinArgs *fin = nullptr, int *n_slots = nullptr, int slot_cap = 0) {
  const L1BwdArgs a = window_gather_args(c);
  if (!fin) return launch_dw_all(j.gg, a, c.basis->basis, c.st, nullptr, nullptr, nullptr, c.ride->bin_next);
  int need = dw_all_knot_blocks(a);
  if (fin->cnt) {
    STDADK_REQUIRE(j.rg.n > 0, STDADK_E_ARG, "dw_all: finishing work without its reduce table");
    for (int i = 0; i < j.gg.n; ++i) need += (int)(ceil_div(j.gg.job[i].M, 64) * ceil_div(j.gg.job[i].N, 64));
    need += reduce_jobs_block_count(j.rg);
  }
  STDADK_REQUIRE(need <= slot_cap, STDADK_E_WORKSPACE, "dw_all: %d squared-norm slots, the plan holds %d", need, slot_cap);
  return launch_dw_all(j.gg, a, c.basis->basis, c.st, fin, fin->cnt ? &j.rg : nullptr, n_slots, c.ride->bin_next);
}

// forward of one batch; training != 0 keeps everything backward needs in the workspace
// (window path: `y`, when given, is carried into sorted order next to the observations, and the
//  predictions stay in sorted order in the plan's ypred buffer; y_pred NULL skips the un-permute).
// `hold` (training step): the row-local launches are filled into it and, where the step's backward can run them inside
// its own row-local launch, left to it (tail_held / l1_held); NULL: everything is issued here.
static int step_forward(const Ctx &c, const float *coords, const float *t, const float *X, const float *y, float *y_pred,
                        Held *hold) {
  const stdadk_mlp_desc *d = c.d;
  const stdadk_basis_desc *b = c.basis;
  float *ws = c.ws;
  Held local;
  Held &h = hold ? *hold : local;
  // one launch for the forward and backward chains of the tail when the loss is fused into it
  const bool can_hold = hold && c.fuse_tail && c.mse_y && fused_tail(c);
  bool is_tail;
  int rc;
  if (c.window) {
    rc = window_layer0_forward(c, coords, t, X, y, h.l1);
    if (rc) return rc;
    // at <= 16 rows per CU layer 0 is held too: layer 0, the tail forward, the loss and the tail backward as ONE kernel
    h.l1_held = can_hold && tail_rows(c.B) == 16 && l1_tail_supported(c.B, h.l1.H) && getenv("STDADK_NO_L1_TAIL") == nullptr;
    if (!h.l1_held) {
      rc = l1_window_forward(h.l1, b->basis, d->layernorm != 0, c.st);
      if (rc) return rc;
    }
    rc = run_forward(c, 1, ws + c.pl.act[0], d->hidden[0], d->hidden[0], ws + c.pl.ypred, nullptr, h.tail, &is_tail);
  } else {
    Dense0Src d0 = {coords, t, X, b->s_bw};
    if (c.log_bw && b->Ks > 0) {        // bandwidth = exp(log_bandwidth)  (st_interp.py:146-148)
      rc = launch_exp(b->s_bw, b->Ks, ws + c.pl.bw_exp, c.st);
      if (rc) return rc;
      d0.s_bw = ws + c.pl.bw_exp;
    }
    if (dense0_in_tail(c)) {
      rc = run_forward(c, 0, nullptr, 0, d->in_dim, y_pred, &d0, h.tail, &is_tail);
    } else {
      rc = stdadk_rbf_build_f32(coords, t, X, c.B, b->p, b->s_centers, d0.s_bw, b->Ks, b->basis, b->t_centers,
                                b->t_bw, b->Kt, ws + c.pl.feats, c.pl.ldf, (stdadk_stream_t)c.st);
      if (rc) return rc;
      rc = run_forward(c, 0, ws + c.pl.feats, c.pl.ldf, d->in_dim, y_pred, nullptr, h.tail, &is_tail);
    }
  }
  if (rc) return rc;
  h.loss_fused = is_tail && c.mse_y != nullptr;
  h.cap32 = is_tail && c.bf16 && h.tail.d0.on != 0;
  h.tail_held = is_tail && can_hold;
  if (is_tail && !h.tail_held) {
    rc = tail_forward(h.tail, c.st);
    if (rc) return rc;
  }
  if (!c.window || !y_pred) return 0;
  return unpermute_rows(ws + c.pl.ypred, (const int *)(ws + c.pl.perm), (int)c.B, d->out_dim, y_pred, c.st);
}

// the knot penalties' checks, shared by the doors that take them
static int check_knot_train(const char *what, const stdadk_knot_train *kt) {
  if (!kt) return 0;
  STDADK_REQUIRE(kt->centers_init || (!kt->gradient_damping && !(kt->movement_weight > 0.f)), STDADK_E_ARG,
                 "%s: centers_init is NULL but damping / movement penalty is on", what);
  STDADK_REQUIRE(kt->domain_weight >= 0.f && kt->movement_weight >= 0.f, STDADK_E_ARG, "%s: negative penalty weight", what);
  return 0;
}

// the knot finish of the batch whose raw per-knot sums sit in the workspace of `c` (kt NULL: the plain data gradient)
static KnotFinishArgs knot_finish_args(const Ctx &c, const stdadk_basis_desc *b, const stdadk_knot_train *kt,
                                       float *d_centers, float *d_log_bw, float *loss_sum) {
  KnotFinishArgs fa;
  fa.part = c.ws + c.pl.kpart; fa.slabs = c.pl.kslabs; fa.Ks = (int)b->Ks; fa.centers = b->s_centers;
  fa.centers_init = kt ? kt->centers_init : nullptr;
  fa.damping = kt ? kt->gradient_damping : 0;
  fa.thr = kt ? kt->damping_threshold : 0.f; fa.strength = kt ? kt->damping_strength : 0.f;
  fa.dom_w = kt ? kt->domain_weight : 0.f; fa.mov_w = kt ? kt->movement_weight : 0.f;
  fa.pen_grad_scale = kt ? kt->penalty_grad_scale : 0.f; fa.pen_loss_scale = kt ? kt->penalty_loss_scale : 0.f;
  fa.d_centers = d_centers; fa.d_log_bw = d_log_bw; fa.loss_sum = loss_sum;
  return fa;
}

// materialising path: the raw per-slab knot sums from dZ of layer 0, which the backward left in the workspace
static int knot_dense_sums(const Ctx &c, const stdadk_basis_desc *b, const stdadk_mlp_tensors *P, const float *coords) {
  const stdadk_mlp_desc *d = c.d;
  float *ws = c.ws;
  const int H = d->hidden[0];
  const float *dz0 = layer0_dz(c);
  // dFeat = dZ0 . W0 over ALL feature columns, into the (now free) feature buffer
  float *dfeat = ws + c.pl.feats;
  int rc;
  if (c.w0t)
    rc = gemm_run(dz0, H, false, P->W[0], H, false, (int)c.B, d->in_dim, H, nullptr, dfeat, c.pl.ldf,
                  ws + c.pl.slab, false, nullptr, c.st);
  else
    rc = gemm_run(dz0, H, false, P->W[0], d->in_dim, true, (int)c.B, d->in_dim, H, nullptr, dfeat, c.pl.ldf,
                  ws + c.pl.slab, false, nullptr, c.st);
  if (rc) return rc;
  KnotGradArgs ka;
  ka.coords = coords; ka.B = (int)c.B; ka.dFeat = dfeat; ka.ld = c.pl.ldf; ka.p = b->p;
  ka.centers = b->s_centers; ka.bw = ws + c.pl.bw_exp; ka.Ks = (int)b->Ks; ka.basis = b->basis;
  ka.part = ws + c.pl.kpart; ka.slabs = c.pl.kslabs;
  return launch_knot_grad(ka, c.st);
}

// "The merged weight-gradient launch applies": window path behind the fused tail, no auxiliary stream to fork the per-knot
// gather onto (environment STDADK_NO_DW_ALL=1: the separate launches, diagnostic)
static bool merged_dw(const Ctx &c) { return c.window && !c.aux && fused_tail(c) && getenv("STDADK_NO_DW_ALL") == nullptr; }

// The finishing mode of the merged weight-gradient launch (FinArgs), decided before the row-local launch, which clears the
// arrival counters for mode 2.  2: the launch also does the reductions -- for large batches, where the K slices of a tile
// arrive spread out and the sums hide under the rest of the launch; below that the last slices arrive together at the
// end of the launch and their sums would extend it by more than the reductions launch costs (measured at 4 096 rows:
// 45 us against 27.6 + 7.7), so 1: the launch only leaves the squared norms of its knot rows.  Environment
// STDADK_DW_FIN=0|1|2 forces a mode (0 = the round-2 path: reductions launch that also re-reads the knot rows for their norm).
static int finishing_mode(const Ctx &c) {
  if (c.pl.fin_cap <= 0) return 0;
  const stdadk_mlp_desc *d = c.d;
  const int64_t t0 = ceil_div(d->hidden[0], 64);
  int64_t tiles = ceil_div(c.basis->Kt, 64) * t0 + (c.basis->p > 0 ? ceil_div(c.basis->p, 64) * t0 : 0);
  for (int l = 1; l < d->n_hidden; ++l) tiles += ceil_div(d->hidden[l], 64) * ceil_div(d->hidden[l - 1], 64);
  const char *e = getenv("STDADK_DW_FIN");
  int fin = e ? atoi(e) : (c.B >= FIN_FULL_MIN_ROWS ? 2 : 1);
  if (fin < 0 || fin > 2) fin = 1;
  if (fin == 2 && tiles > FIN_TILES_MAX) fin = 1;
  return fin;
}

// Closes the weight gradients of a step behind the dZ launch: issues whatever is still to launch of `jobs` (NULL: the
// generic kernels left nothing pending) and of the per-knot gather, lets the step's riders (c.ride) ride, and says in
// `out` where the clip-norm partials went and whether the next batch is binned.  `merged`: merged_dw(c), which `fin`
// was decided from.  Who leaves the partials also advances the step counter (ride.step_inc); when nobody
// does (out.sq_parts NULL) the caller's own norm pass or stdadk_step_advance does.  A learnable one-call step
// (ride.knots) passes no step_inc: its finishing launch (step_finish.hip) is in every case and advances finish_inc.
//
//   case                                    launches                                    partials + step_inc ride in
//   merged dW launch, finishing mode 2      dw_all                                      dw_all (its slots)
//   merged dW launch, finishing mode 1      dw_all, reductions                          dw_all (knot rows) + reductions
//   merged dW launch, finishing mode 0      dw_all, reductions                          reductions (+ its 256 region workgroups)
//   separate launches (auxiliary stream,    grouped GEMMs, reductions, dW0 GEMM /       reductions, on the materialising path when
//     STDADK_NO_DW_ALL, materialising path)   per-knot gather (or its join)               every gradient is its output; else nobody
//   learnable, reductions pending (0 / 1)   the finishing launch in the reductions' place, carrying their jobs (mode 0's
//                                           region workgroups stay a reductions launch of their own)
//   learnable, nothing pending (mode 2,     the finishing launch with zero reduce workgroups, last
//     separate launches, generic kernels)
//   delta head (ride.head)                  always ends in the finishing launch, learnable or not, whose LAST workgroup is
//                                           the head's: it runs the output layer's two sums itself where the fused tail
//                                           left them as column partials (they are in no reduce table then and leave no
//                                           squares) and adds ONE slot behind the others.  Fixed knots: the launch also
//                                           stands in for the reductions launch of the separate launches' row
static int close_step(const Ctx &c, DwJobs *jobs, bool merged, int fin, const float *coords, StepOut &out) {
  const StepRide &r = *c.ride;
  float *ws = c.ws;
  const stdadk_basis_desc *b = c.basis;
  const bool forked = jobs && c.aux;      // window path: the per-knot gather already runs on the auxiliary stream
  const bool sq = jobs && r.gradsq_parts && jobs->all_grouped;
  const int nrb = jobs ? reduce_jobs_block_count(jobs->rg) : 0;
  const bool fin_launch = r.knots || r.head;    // the step ends in the finishing launch
  const int hs = r.head ? 1 : 0;                // the head workgroup's ONE slot behind the others
  float *head_slot = nullptr;
  // the output layer's jobs where they stayed in the table (head_sums_pending false): the first two, their squares in
  // the first nhb slots of the reduce / tall workgroups
  const bool head_in_table = r.head && jobs && !jobs->head_apart;
  const int nhb = head_in_table ? jobs->rg.first_block[2] : 0;
  float *head_zero = nullptr;
  bool reductions_pending = false;
  int rc = 0;
  if (merged && fin == 2) {
    // products, per-knot gather, every fixed-order sum and the squared-norm partials: ONE launch
    FinArgs f;
    f.cnt = reinterpret_cast<int *>(ws + c.pl.fin_cnt);
    f.slots = sq ? ws + c.pl.fin_slots : nullptr;
    f.step_inc = sq ? r.step_inc : nullptr;
    int n_slots = 0;
    rc = window_dw_all(c, *jobs, &f, &n_slots, c.pl.fin_cap - hs);
    if (sq) { out.sq_parts = f.slots; out.sq_n = n_slots + hs; head_slot = f.slots + n_slots; }
    if (sq && head_in_table) {      // the tall workgroups' slots start behind the output tiles'
      int nt = 0;
      for (int i = 0; i < jobs->gg.n; ++i) nt += (int)(ceil_div(jobs->gg.job[i].M, 64) * ceil_div(jobs->gg.job[i].N, 64));
      head_zero = f.slots + nt;
    }
  } else if (merged && fin == 1 && sq && nrb > 0) {
    // the knot workgroups leave the squares of the rows they write (no second pass over dW0^T), the reductions
    // launch adds the partials of what it writes behind them
    FinArgs f;
    f.slots = ws + c.pl.fin_slots;
    int n_knot = 0;
    rc = window_dw_all(c, *jobs, &f, &n_knot, c.pl.fin_cap - nrb - hs);
    jobs->rg.sq_parts = f.slots + n_knot;
    jobs->rg.step_inc = r.step_inc;
    out.sq_parts = f.slots; out.sq_n = n_knot + nrb + hs; head_slot = f.slots + n_knot + nrb;
    reductions_pending = true;
  } else if (merged) {
    rc = window_dw_all(c, *jobs);
    if (rc) return rc;
    if (sq && nrb > 0 && nrb <= STDADK_GRADSQ_PARTS - 256 - hs) {
      // every gradient of the step is either an output of the reductions launch or a spatial row of dW0^T (final
      // after the launch above): their squared norm comes out of the same launch
      ReduceGroup own;
      ReduceGroup &region = fin_launch ? own : jobs->rg;
      region.sq_region_parts = r.gradsq_parts;
      region.sq_src = c.G->W[0] + (size_t)b->p * c.d->hidden[0];
      region.sq_n = (int64_t)b->Ks * c.d->hidden[0];
      if (fin_launch) rc = launch_reduce_jobs(region, c.st);
      jobs->rg.sq_parts = r.gradsq_parts + 256;
      jobs->rg.step_inc = r.step_inc;
      out.sq_parts = r.gradsq_parts; out.sq_n = 256 + nrb + hs; head_slot = r.gradsq_parts + 256 + nrb;
    }
    reductions_pending = true;
  } else if (jobs) {
    if (sq && !c.window && jobs->dw0_in_group && nrb > 0 && nrb <= STDADK_GRADSQ_PARTS - hs) {
      // one-call step: every gradient of the step is an output of this reductions launch, which then also
      // leaves the squared-norm partials for the clip (no region beside them)
      jobs->rg.sq_parts = r.gradsq_parts; jobs->rg.step_inc = r.step_inc;
      out.sq_parts = r.gradsq_parts; out.sq_n = nrb + hs; head_slot = r.gradsq_parts + nrb;
      if (head_in_table) head_zero = r.gradsq_parts;
    }
    // (a fixed-knot delta step: the finishing launch stands where the reductions launch stood and carries its jobs)
    reductions_pending = r.head && !r.knots;
    rc = launch_dw_jobs(c, *jobs, c.window ? nullptr : ws + c.pl.feats, c.pl.ldf, !reductions_pending);
  }
  if (rc) return rc;
  if (merged) out.binned_next = r.bin_next != nullptr;
  if (c.window && !merged) {
    rc = forked ? stream_depends(c.st, c.aux, 3) : window_gather(c, c.st);      // join | the gather, last
    if (rc) return rc;
  }
  if (reductions_pending && !fin_launch) return launch_reduce_jobs(jobs->rg, c.st);
  if (!fin_launch) return 0;
  // the per-knot sums are final: once the dW launch is (window path), or from dZ of layer 0 here (materialising path)
  if (r.knots && !c.window) {
    rc = knot_dense_sums(c, b, c.P, coords);
    if (rc) return rc;
  }
  HeadFinishArgs hf;
  if (r.head) {
    // the output layer's sums: still column partials behind the fused tail kernels (the head workgroup runs them),
    // final behind the generic kernels (head_reduce / GEMM + colsum)
    hf = *r.head;
    hf.sq_part = head_slot;
    hf.pending = jobs && jobs->head_apart ? 1 : 0;
    if (hf.pending) { hf.job[0] = jobs->head_job[0]; hf.job[1] = jobs->head_job[1]; }
    hf.zero_slots = head_zero; hf.n_zero = head_zero ? nhb : 0;
  }
  KnotFinishArgs fa{};
  if (r.knots) fa = knot_finish_args(c, b, r.kt, r.d_centers, r.d_log_bw, c.mse_loss);
  ReduceGroup none;
  return launch_step_finish(reductions_pending ? jobs->rg : none, fa, r.knots ? r.knot_sq : nullptr, r.finish_inc, c.st,
                            r.head ? &hf : nullptr);
}

// Delta step behind the fused tail kernels: are the output layer's two fixed-order sums still pending when the
// finishing launch starts?  No where a launch in front of it runs reduce jobs anyway -- the weight-gradient launch in
// finishing mode 2 (its tall workgroups), the reductions launch of a learnable step's separate launches (materialising
// route) -- : the sums stay in the table there, the head workgroup reads them and clears their slots of squares.  Yes
// where the finishing launch itself carries the reductions (window modes 0 / 1, fixed-knot separate launches): there
// they leave the table and the head workgroup runs them (close_step).
static bool head_sums_pending(const Ctx &c, bool merged, int fin) {
  if (!c.ride->head) return false;
  return merged ? fin != 2 : !c.ride->knots;
}

// backward of the batch whose training forward left its state in the workspace; dY in caller order
// (`dY_sorted`: window path only — dY is already the plan's dY buffer in sorted order); `h`: what that forward held
// back (NULL: nothing, a split call); `coords`: the batch's, for the knot sums of a learnable one-call step on the
// materialising path
static int step_backward(const Ctx &c, const float *dY, bool dY_sorted, Held *h, const float *coords, StepOut &out) {
  const stdadk_mlp_desc *d = c.d;
  const stdadk_basis_desc *b = c.basis;
  float *ws = c.ws;
  const bool fused = fused_tail(c);
  int64_t n_part;
  DwJobs jobs;
  int rc;
  if (!c.window) {
    if (!fused) {
      rc = generic_backward(c, dY, ws + c.pl.feats, c.pl.ldf, true);
      if (rc) return rc;
      return close_step(c, nullptr, false, 0, coords, out);
    }
    rc = tail_row_launch(c, dY, true, 0, h, &n_part);
    if (rc) return rc;
    rc = collect_dw_jobs(c, n_part, 0, nullptr, 0, ws + c.pl.feats, c.pl.ldf, jobs, head_sums_pending(c, false, 0));
    if (rc) return rc;
    return close_step(c, &jobs, false, 0, coords, out);
  }
  const int H = d->hidden[0], Q = d->out_dim;
  if (!dY_sorted) {   // dY rows into sorted order
    STDADK_LAUNCH(gather_rows_kernel, dim3((unsigned)ceil_div(c.B * Q, 256)), dim3(256), 0, c.st, dY,
                       (const int *)(ws + c.pl.perm), (int)c.B, Q, ws + c.pl.dY);
    STDADK_CHECK_LAUNCH("gather_rows");
  }
  // dW0^T rows of the temporal / covariate columns: small products that ride along with the dW
  // GEMMs of the fused-tail backward (or run on their own on the generic path)
  ExtraProduct extra[2];
  int n_extra = 0;
  extra[n_extra++] = {ws + c.pl.psi, c.pl.ld_psi, (int)b->Kt, c.G->W[0] + (size_t)(b->p + b->Ks) * H};
  if (b->p > 0) extra[n_extra++] = {ws + c.pl.X_s, b->p, b->p, c.G->W[0]};
  STDADK_REQUIRE(c.G->W[0], STDADK_E_ARG, "backward: dW[0] NULL");
  if (!fused) {
    rc = generic_backward(c, ws + c.pl.dY, nullptr, 0, false);
    if (rc) return rc;
    for (int e = 0; e < n_extra; ++e) {
      rc = gemm_run(extra[e].A, extra[e].lda, true, layer0_dz(c), H, true, extra[e].M, H, (int)c.B, nullptr,
                    extra[e].C, H, ws + c.pl.slab, false, nullptr, c.st);
      if (rc) return rc;
    }
    return close_step(c, nullptr, false, 0, coords, out);
  }
  const bool merged = merged_dw(c);
  const int fin = merged ? finishing_mode(c) : 0;
  rc = tail_row_launch(c, ws + c.pl.dY, false, fin, h, &n_part);
  if (rc) return rc;
  if (c.aux) {
    // dZ is final: the knot-row gather of dW0^T runs on the auxiliary stream beside the dW GEMMs and reductions of
    // the other layers
    rc = stream_depends(c.aux, c.st, 2);
    if (rc) return rc;
    rc = window_gather(c, c.aux);
    if (rc) return rc;
  }
  rc = collect_dw_jobs(c, n_part, fin, extra, n_extra, nullptr, 0, jobs, head_sums_pending(c, merged, fin));
  if (rc) return rc;
  return close_step(c, &jobs, merged, fin, coords, out);
}

extern "C" int stdadk_forward_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                  const stdadk_mlp_tensors *P, const float *coords, const float *t,
                                  const float *X, int64_t B, float *y_pred, void *workspace,
                                  size_t workspace_bytes, int32_t training, uint64_t drop_seed,
                                  const int32_t *step_dev, int32_t flags, stdadk_stream_t stream) {
  if (B == 0) return 0;
  Ctx c;
  int rc = open_step(c, b, d, B, workspace, workspace_bytes, flags, P, nullptr, stream, training != 0, drop_seed, step_dev);
  if (rc) return rc;
  STDADK_REQUIRE(P && coords && t && y_pred, STDADK_E_ARG, "forward: NULL pointer");
  STDADK_REQUIRE(b->p == 0 || X, STDADK_E_ARG, "forward: X is NULL with p=%d", b->p);
  return step_forward(c, coords, t, X, nullptr, y_pred, nullptr);
}

// ---------------------------------------------------------------------------------------------------------
// Site x time prediction grids (A10): layer 0's pre-activation splits into a per-site and a per-time row
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void temporal_partial_kernel(const float *__restrict__ tv, int T, int Kt,
                                                               const float *__restrict__ tc, const float *__restrict__ tbw,
                                                               const float *__restrict__ Wt, int H, float *__restrict__ out) {
  // out[ti][c] = sum_j psi_j(t_ti) Wt[j][c]; one workgroup per time value
  const int ti = blockIdx.x;
  const float t = tv[ti];
  for (int c = threadIdx.x; c < H; c += 256) {
    float acc = 0.f;
    for (int j = 0; j < Kt; ++j) acc = fmaf(psi_eval(t, tc[j], tbw[j]), Wt[(size_t)j * H + c], acc);
    out[(size_t)ti * H + c] = acc;
  }
}

extern "C" int stdadk_spatial_partial_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                          const stdadk_mlp_tensors *P, const float *coords, int64_t S, float *out,
                                          void *workspace, size_t workspace_bytes, int32_t flags,
                                          stdadk_stream_t stream) {
  if (S == 0) return 0;
  Ctx c;
  // (`training` false: this door reads neither dp nor save)
  int rc = open_step(c, b, d, S, workspace, workspace_bytes, flags, P, nullptr, stream, false);
  if (rc) return rc;
  STDADK_REQUIRE(c.window && !(flags & STDADK_FLAG_LOG_BW), STDADK_E_ARG,
                 "spatial_partial: needs the window path with fixed grid knots (compact-support basis, W0 stored (in,out))");
  STDADK_REQUIRE(b->p == 0, STDADK_E_ARG, "spatial_partial: covariates are per (site, time) row; p must be 0");
  STDADK_REQUIRE(P && P->W[0] && P->b[0] && coords && out, STDADK_E_ARG, "spatial_partial: NULL pointer");
  const Plan &pl = c.pl;
  BinBuffers bb = plan_bins(c.ws, pl);
  // the sites' x coordinates stand in for the (unused) time column of the binning
  rc = bin_obs(coords, coords, nullptr, 0, nullptr, 0, (int)S, pl.G, bb, c.st);
  if (rc) return rc;
  L1FwdArgs a;
  a.g = make_grid(b, c.scattered);
  a.halo = nullptr;
  if (c.scattered) {
    rc = scattered_bins(c, a);
    if (rc) return rc;
  }
  a.xs = bb.xs; a.ys = bb.ys; a.ts = bb.ts; a.Xs = nullptr;
  a.B = (int)S; a.H = d->hidden[0];
  a.W0T = P->W[0]; a.b0 = P->b[0]; a.gamma = a.beta = nullptr; a.eps = d->ln_eps;
  a.xhat = a.rstd = a.psi = nullptr; a.ld_psi = pl.ld_psi;
  a.act = c.ws + pl.act[0];
  a.drop_p = 0.f; a.seed = 0; a.step_dev = nullptr;
  a.rows_per_wg = 0; a.n_wg = 0;
  a.raw = 1;
  rc = l1_window_forward(a, b->basis, false, c.st);
  if (rc) return rc;
  return unpermute_rows(c.ws + pl.act[0], (const int *)(c.ws + pl.perm), (int)S, d->hidden[0], out, c.st);
}

extern "C" int stdadk_temporal_partial_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                           const stdadk_mlp_tensors *P, const float *t_values, int64_t T,
                                           float *out, int32_t flags, stdadk_stream_t stream) {
  if (T == 0) return 0;
  int rc = check_desc(d);
  if (rc) return rc;
  STDADK_REQUIRE(b && P && P->W[0] && t_values && out && T < (1ll << 31), STDADK_E_ARG, "temporal_partial: bad argument");
  STDADK_REQUIRE((flags & STDADK_FLAG_W0_T) && d->n_hidden >= 1, STDADK_E_ARG,
                 "temporal_partial: needs the first weight stored (in,out)");
  const int H = d->hidden[0];
  STDADK_LAUNCH(temporal_partial_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, t_values, (int)T,
                (int)b->Kt, b->t_centers, b->t_bw, P->W[0] + (size_t)(b->p + b->Ks) * H, H, out);
  STDADK_CHECK_LAUNCH("temporal_partial");
  return 0;
}

// the shapes stdadk_forward_parts_f32 runs: the fused tail from layer 0 on (the query and the door share this)
static bool forward_parts_shape_ok(const stdadk_mlp_desc *d) { return d->n_hidden >= 1 && tail_supported(d, 1); }

extern "C" int32_t stdadk_forward_parts_supported(const stdadk_mlp_desc *d) {
  if (check_desc(d) != 0) return 0;
  return forward_parts_shape_ok(d) ? 1 : 0;
}

extern "C" int stdadk_forward_parts_f32(const stdadk_mlp_desc *d, const stdadk_mlp_tensors *P, const float *sp,
                                        int64_t S, const float *tp, int64_t T, float *y_pred,
                                        stdadk_stream_t stream) {
  if (S == 0 || T == 0) return 0;
  int rc = check_desc(d);
  if (rc) return rc;
  const int L = d->n_hidden;
  STDADK_REQUIRE(P && sp && tp && y_pred && S * T < (1ll << 31), STDADK_E_ARG, "forward_parts: bad argument");
  STDADK_REQUIRE(forward_parts_shape_ok(d) && P->W[L] && P->b[L], STDADK_E_ARG,
                 "forward_parts: hidden widths must be multiples of 16 up to %d, out_dim <= %d", TAIL_MAX_W, TAIL_MAXQ);
  TailFwdArgs a;
  a.n_layers = L - 1;
  for (int l = 1; l < L; ++l) {
    STDADK_REQUIRE(P->W[l] && P->b[l] && (!d->layernorm || (P->ln_g[l] && P->ln_b[l])), STDADK_E_ARG,
                   "forward_parts: layer %d parameters NULL", l);
    a.L[l - 1] = tail_layer(d, P, true, l);
  }
  STDADK_REQUIRE(P->b[0] && (!d->layernorm || (P->ln_g[0] && P->ln_b[0])), STDADK_E_ARG, "forward_parts: layer 0 parameters NULL");
  a.d0.on = 2; a.d0.sp = sp; a.d0.tp = tp; a.d0.S = (int)S;
  a.d0.L0 = tail_layer(d, P, true, 0);
  a.a_in = nullptr; a.h_in = d->hidden[0];
  a.B = (int)(S * T);
  tail_fwd_model(a, d, P);
  a.y_pred = y_pred;
  a.drop_p = 0.f; a.seed = 0; a.step_dev = nullptr; a.stamps = nullptr;
  // bf16 operands whenever the caller supplies the copies of every layer after the first
  a.bf16 = L > 1 ? 1 : 0;
  for (int l = 1; l < L; ++l) if (!P->W_bf16[l]) a.bf16 = 0;
  return tail_forward(a, (hipStream_t)stream);
}

extern "C" int stdadk_backward_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                   const stdadk_mlp_tensors *P, const stdadk_mlp_tensors *G, int64_t B,
                                   const float *dY, void *workspace, size_t workspace_bytes,
                                   uint64_t drop_seed, const int32_t *step_dev, int32_t flags,
                                   stdadk_stream_t stream) {
  if (B == 0) return 0;
  Ctx c;
  int rc = open_step(c, b, d, B, workspace, workspace_bytes, flags, P, G, stream, true, drop_seed, step_dev);
  if (rc) return rc;
  STDADK_REQUIRE(P && G && dY, STDADK_E_ARG, "backward: NULL pointer");
  StepOut out;
  return step_backward(c, dY, false, nullptr, nullptr, out);
}

extern "C" int stdadk_knot_backward_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                        const stdadk_mlp_tensors *P, const float *coords, int64_t B,
                                        void *workspace, size_t workspace_bytes, int32_t flags,
                                        const stdadk_knot_train *kt, float *d_centers, float *d_log_bw,
                                        float *loss_sum, stdadk_stream_t stream) {
  if (B == 0) return 0;
  Ctx c;
  // (`training` false: this door reads neither dp nor save)
  int rc = open_step(c, b, d, B, workspace, workspace_bytes, flags, P, nullptr, stream, false);
  if (rc) return rc;
  STDADK_REQUIRE((flags & STDADK_FLAG_LOG_BW), STDADK_E_ARG,
                 "knot_backward: needs STDADK_FLAG_LOG_BW (the state of a learnable-knot forward/backward)");
  STDADK_REQUIRE(P && P->W[0] && (coords || c.window) && d_centers && d_log_bw, STDADK_E_ARG,
                 "knot_backward: NULL pointer");
  STDADK_REQUIRE(b->Ks > 0 && d->n_hidden >= 1, STDADK_E_ARG, "knot_backward: no spatial knots / no hidden layer");
  rc = check_knot_train("knot_backward", kt);
  if (rc) return rc;
  const KnotFinishArgs fa = knot_finish_args(c, b, kt, d_centers, d_log_bw, loss_sum);
  // window path: the per-knot gather of the backward already left the raw sums in the workspace
  if (!c.window) {
    rc = knot_dense_sums(c, b, P, coords);
    if (rc) return rc;
  }
  return launch_knot_finish(fa, c.st);
}

// where a step's predictions land: the plan's buffer (window path: sorted order, y_pred gets the un-permuted copy)
static float *pred_buffer(const Ctx &c, float *y_pred) { return (c.window || !y_pred) ? c.ws + c.pl.ypred : y_pred; }

// the loss of a step on predictions `yp` where no tail launch fused it: c.mse_y -> c.mse_dY / c.mse_loss, as the tail does
static int launch_step_loss(const Ctx &c, const float *yp) {
  const int Q = c.d->out_dim;
  if (loss_is_plain_mse(c.loss, Q)) return launch_mse(yp, c.mse_y, c.B * Q, c.mse_scale, c.mse_dY, c.mse_loss, c.st);
  return launch_loss(c.loss, yp, c.mse_y, c.B, Q, c.mse_scale, c.mse_dY, c.mse_loss, c.st);
}

// what every training door fills alike
static StepCall step_call(const stdadk_basis_desc *b, const stdadk_mlp_desc *d, const stdadk_mlp_tensors *P,
                          const stdadk_mlp_tensors *G, const float *coords, const float *t, const float *X, const float *y,
                          int64_t B, float grad_scale, const stdadk_loss_desc *loss, float *loss_sum, void *workspace,
                          size_t workspace_bytes, uint64_t drop_seed, int32_t flags, stdadk_stream_t stream) {
  StepCall s;
  s.b = b; s.d = d; s.P = P; s.G = G; s.coords = coords; s.t = t; s.X = X; s.y = y; s.B = B;
  s.grad_scale = grad_scale; s.loss = loss; s.loss_sum = loss_sum; s.workspace = workspace;
  s.workspace_bytes = workspace_bytes; s.drop_seed = drop_seed; s.flags = flags; s.stream = stream;
  return s;
}

// forward, loss and backward of one batch; `ride` / `out`: one-call step only (an error return leaves {NULL, 0, false})
static int train_fwd_bwd_impl(const StepCall &s, const StepRide *ride, StepOut *out) {
  if (out) *out = StepOut{};
  if (s.B == 0) return 0;
  const stdadk_basis_desc *b = s.b;
  Ctx c;
  int rc = open_step(c, b, s.d, s.B, s.workspace, s.workspace_bytes, s.flags, s.P, s.G, s.stream, true, s.drop_seed,
                     s.step_dev);
  if (rc) return rc;
  STDADK_REQUIRE(!s.idx || c.window, STDADK_E_ARG,
                 "train_fwd_bwd_indexed: only the window path gathers in place; use stdadk_gather_batch_f32 + "
                 "stdadk_train_fwd_bwd_f32 for the materialising path");
  c.idx = s.idx;
  if (ride) c.ride = ride;
  STDADK_REQUIRE(s.P && s.G && (c.prebinned || (s.coords && s.t && s.y)), STDADK_E_ARG, "train_fwd_bwd: NULL pointer");
  c.aux = (s.aux_stream && s.aux_stream != s.stream) ? (hipStream_t)s.aux_stream : nullptr;
  STDADK_REQUIRE(b->p == 0 || s.X || c.prebinned, STDADK_E_ARG, "train_fwd_bwd: X is NULL with p=%d", b->p);
  rc = make_loss(s.loss, s.d->out_dim, &c.loss);
  if (rc) return rc;
  // window path: predictions, targets and dY stay in sorted order between the binning and the weight gradients
  float *yp = pred_buffer(c, s.y_pred);
  c.mse_y = c.window ? c.ws + c.pl.y_s : s.y; c.mse_scale = s.grad_scale; c.mse_dY = c.ws + c.pl.dY; c.mse_loss = s.loss_sum;
  // the forward may hold its row-local launches back for the backward's when nothing has to read the predictions
  // in between (window path: the un-permute of y_pred)
  c.fuse_tail = getenv("STDADK_NO_TAIL_FWD_BWD") == nullptr && !(c.window && s.y_pred);
  // ---- from here on `c` is read-only: forward -> (loss) -> backward, what they hand on by value
  Held held;
  StepOut left;
  if (c.ride->head) {     // delta step: the output layer of this step's delta, the call's first launch
    const HeadFinishArgs &hd = *c.ride->head;
    rc = launch_delta_head(hd.delta, hd.ldd, hd.Q, hd.d, s.P->W[s.d->n_hidden], s.P->b[s.d->n_hidden], c.st);
    if (rc) return rc;
  }
  rc = step_forward(c, s.coords, s.t, s.X, s.y, c.window ? s.y_pred : yp, &held);
  if (rc) return rc;
  if (!held.loss_fused) {
    rc = launch_step_loss(c, yp);
    if (rc) return rc;
  }
  rc = step_backward(c, c.mse_dY, c.window, &held, s.coords, left);
  if (rc) return rc;
  STDADK_REQUIRE(!c.window || (!held.tail_held && !held.l1_held), STDADK_E_ARG, "train_fwd_bwd: a parked launch was never issued");
  STDADK_REQUIRE(c.window || !held.tail_held, STDADK_E_ARG, "train_fwd_bwd: the parked tail launch was never issued");
  if (out) *out = left;
  return 0;
}

// the second parameter group of a one-call step (stdadk_train_step_knots_f32): the learnable knots
struct KnotStep {
  const stdadk_knot_train *kt = nullptr;
  float *d_centers = nullptr, *d_log_bw = nullptr;
  const stdadk_adam_group *group = nullptr;
};

// what the knots door refuses before anything is planned: flags, the knot group, where its gradients go, the penalties
static int check_knot_step(const char *door, const StepCall &s, const KnotStep &k) {
  const stdadk_basis_desc *b = s.b; const stdadk_mlp_desc *d = s.d;
  STDADK_REQUIRE(b && d, STDADK_E_ARG, "%s: basis / mlp descriptor is NULL", door);
  STDADK_REQUIRE((s.flags & STDADK_FLAG_LOG_BW), STDADK_E_ARG,
                 "%s: flags need STDADK_FLAG_LOG_BW (learnable knots: basis->s_bw holds log-bandwidths)", door);
  STDADK_REQUIRE(!(s.flags & STDADK_FLAG_PACK_F32), STDADK_E_ARG,
                 "%s: flags carry STDADK_FLAG_PACK_F32; packed fp32 copies are not kept on this path", door);
  STDADK_REQUIRE(b->Ks > 0 && b->Ks < (1ll << 31) && d->n_hidden >= 1, STDADK_E_ARG,
                 "%s: no spatial knots / no hidden layer", door);
  const stdadk_adam_group *g = k.group;
  STDADK_REQUIRE(g && g->p && g->g && g->m && g->v && g->n > 0, STDADK_E_ARG, "%s: knots group incomplete", door);
  STDADK_REQUIRE(!g->shadow, STDADK_E_ARG, "%s: knots->shadow must be NULL (the knot group has no operand copies)", door);
  STDADK_REQUIRE(g->max_norm <= 0.f || g->sumsq_parts, STDADK_E_ARG,
                 "%s: knots->max_norm > 0 needs knots->sumsq_parts (STDADK_SUMSQ_PARTS floats)", door);
  STDADK_REQUIRE(k.d_centers && k.d_log_bw, STDADK_E_ARG, "%s: d_centers / d_log_bw is NULL", door);
  const float *lo = g->g, *hi = g->g + g->n;
  STDADK_REQUIRE(k.d_centers >= lo && k.d_centers + 2 * b->Ks <= hi, STDADK_E_ARG,
                 "%s: d_centers [Ks,2] lies outside the knot group's gradient range [knots->g, knots->g + n)", door);
  STDADK_REQUIRE(k.d_log_bw >= lo && k.d_log_bw + b->Ks <= hi, STDADK_E_ARG,
                 "%s: d_log_bw [Ks] lies outside the knot group's gradient range [knots->g, knots->g + n)", door);
  STDADK_REQUIRE(s.P && s.P->W[0], STDADK_E_ARG, "%s: params->W[0] is NULL", door);
  char what[64];
  snprintf(what, sizeof what, "%s: kt", door);
  return check_knot_train(what, k.kt);
}

// what the delta door refuses on top: the head's rows, where its gradient goes, the output layer's scratch
static int check_delta_step(const StepCall &s, const stdadk_optim_desc *o, const stdadk_delta_step *h) {
  const stdadk_mlp_desc *d = s.d;
  STDADK_REQUIRE(s.b && d, STDADK_E_ARG, "train_step_delta: basis / mlp descriptor is NULL");
  STDADK_REQUIRE(h && h->delta && h->d_delta, STDADK_E_ARG, "train_step_delta: head is NULL / incomplete");
  STDADK_REQUIRE(d->n_hidden >= 1 && d->n_hidden <= STDADK_MAX_HIDDEN, STDADK_E_ARG, "train_step_delta: no hidden layer");
  const int L = d->n_hidden, Q = d->out_dim, dl = d->hidden[L - 1];
  STDADK_REQUIRE(Q >= 2 && Q <= STDADK_MAX_Q, STDADK_E_ARG, "train_step_delta: Q=%d outside 2..%d (the delta head has Q >= 2 rows)",
                 Q, STDADK_MAX_Q);
  STDADK_REQUIRE(h->ldd >= dl + 1, STDADK_E_ARG, "train_step_delta: ldd=%lld below d + 1 = %d", (long long)h->ldd, dl + 1);
  STDADK_REQUIRE(h->ldg == h->ldd, STDADK_E_ARG, "train_step_delta: the strides of delta (%lld) and d_delta (%lld) differ",
                 (long long)h->ldd, (long long)h->ldg);
  const int64_t span = (int64_t)(Q - 1) * h->ldd + dl + 1;
  STDADK_REQUIRE(h->delta >= o->p && h->delta + span <= o->p + o->n, STDADK_E_ARG,
                 "train_step_delta: delta [Q,ldd] lies outside the parameter range [opt->p, opt->p + n)");
  STDADK_REQUIRE(h->d_delta >= o->g && h->d_delta + span <= o->g + o->n, STDADK_E_ARG,
                 "train_step_delta: d_delta [Q,ldd] lies outside the gradient range [opt->g, opt->g + n)");
  STDADK_REQUIRE(h->d_delta - o->g == h->delta - o->p, STDADK_E_ARG,
                 "train_step_delta: d_delta sits at another offset of the gradient than delta of the parameters");
  STDADK_REQUIRE(s.P && s.G && s.P->W[L] && s.P->b[L] && s.G->W[L] && s.G->b[L], STDADK_E_ARG,
                 "train_step_delta: the derived output layer (params->W[L], b[L]) or its gradient scratch is NULL");
  const float *gw = s.G->W[L], *gb = s.G->b[L], *lo = o->g, *hi = o->g + o->n;
  STDADK_REQUIRE((gw + (int64_t)Q * dl <= lo || gw >= hi) && (gb + Q <= lo || gb >= hi), STDADK_E_ARG,
                 "train_step_delta: grads->W[L] / b[L] (scratch of the derived output layer) lie inside the gradient range "
                 "[opt->g, opt->g + n)");
  return 0;
}

// forward / backward of `s`, sparsity penalty, clip norm, AdamW + EMA; `nb`, when complete, is binned along the way.
// `ks`: the step has a second parameter group, the learnable knots -- their finish rides in the step's finishing
// launch (step_finish.hip), both groups are stepped by one two-group AdamW launch, and the next batch is binned by
// the weight-gradient launch or not at all.
// `ds`: the delta head -- the derived output layer is rebuilt in front, the head workgroup of the finishing launch
// folds its gradient into the delta rows of the flat gradient; with or without `ks`.
static int train_step_impl(StepCall s, const stdadk_sparsity_desc *sparsity, const stdadk_optim_desc *o,
                           const NextBatch &nb, const KnotStep *ks = nullptr, const stdadk_delta_step *ds = nullptr,
                           const char *door = "train_step_knots") {
  const stdadk_basis_desc *b = s.b; const stdadk_mlp_desc *d = s.d;
  if (nb.binned) *nb.binned = 0;
  STDADK_REQUIRE(o && o->p && o->g && o->m && o->v && o->n > 0 && o->step_dev, STDADK_E_ARG,
                 "train_step: optimiser descriptor incomplete");
  STDADK_REQUIRE(o->max_norm <= 0.f || o->sumsq_parts, STDADK_E_ARG, "train_step: max_norm > 0 needs sumsq_parts");
  if (ks) {
    const int rc = check_knot_step(door, s, *ks);
    if (rc) return rc;
  }
  if (ds) {
    const int rc = check_delta_step(s, o, ds);
    if (rc) return rc;
  }
  if (s.B == 0) return 0;
  s.step_dev = o->step_dev;
  // the NEXT batch is validated and planned before anything of this step is enqueued: a call that fails on it
  // leaves the parameters, moments, EMA, step counter and loss sum as they were
  Ctx cn;
  bool bin_next = false;
  if (nb.idx && nb.B > 0 && nb.workspace && nb.binned) {
    int rc = open_step(cn, b, d, nb.B, nb.workspace, nb.workspace_bytes, s.flags & ~STDADK_FLAG_PREBINNED, nullptr, nullptr,
                       s.stream, false);   // planned only: cn.pl, cn.ws and cn.window are read
    if (rc) return rc;
    bin_next = cn.window && bin_small_eligible((int)nb.B, cn.pl.G) && s.coords && s.t && (b->p == 0 || s.X);
    STDADK_REQUIRE(!bin_next || (nb.y_cols >= 0 && nb.y_cols <= d->out_dim && (nb.y_cols == 0 || s.y)),
                   STDADK_E_ARG, "train_step: next_y_cols=%d must be in 0..Q with y given", nb.y_cols);
  }
  // its carrier: the merged weight-gradient launch of this step (dw_all.hip), which has the time and the idle HBM for
  // the binning's chain of dependent loads, whenever that launch is what the step runs and can hold the batch;
  // otherwise, or with STDADK_BIN_IN=adam (diagnostic), the optimiser launch (optim.hip: adamw_bin_kernel).  The
  // weight-gradient launch still reads this step's workspace, so there the next batch must go to another one.
  BinSmallArgs ba{};
  bool bin_in_dw = false;
  if (bin_next) {
    const BinBuffers bb = plan_bins(cn.ws, cn.pl);
    ba = bin_small_args(s.coords, s.t, nb.y_cols > 0 ? s.y : nullptr, nb.y_cols, s.X, b->p, (int)nb.B, cn.pl.G, bb, nb.idx);
    const char *ws0 = (const char *)s.workspace, *ws1 = (const char *)nb.workspace;
    const bool apart = ws1 + nb.workspace_bytes <= ws0 || ws0 + s.workspace_bytes <= ws1;
    const char *e = getenv("STDADK_BIN_IN");
    const bool in_adam = e && e[0] == 'a';
    bin_in_dw = !in_adam && apart && dw_all_bins((int)nb.B, cn.pl.G);
  }
  const bool clip = o->max_norm > 0.f;
  const bool sparse = sparsity && sparsity->kind != STDADK_SPARSITY_NONE;
  // with a sparsity penalty the gradient changes once more after the reductions: the norm is a pass of its own
  const bool fuse_sq = clip && !sparse;
  StepRide ride = {fuse_sq ? o->sumsq_parts : nullptr, fuse_sq ? o->step_dev : nullptr, bin_in_dw ? &ba : nullptr};
  if (ks) {
    // the finishing launch is in every learnable step and advances the counter; no other launch of the step does
    ride.step_inc = nullptr;
    ride.knots = true; ride.kt = ks->kt; ride.d_centers = ks->d_centers; ride.d_log_bw = ks->d_log_bw;
    ride.knot_sq = ks->group->max_norm > 0.f ? const_cast<float *>(ks->group->sumsq_parts) : nullptr;
    ride.finish_inc = o->step_dev;
  }
  HeadFinishArgs head;
  if (ds) {
    // a delta step ends in the finishing launch too, which then advances the counter
    const int L = d->n_hidden;
    head.d_delta = ds->d_delta; head.delta = ds->delta; head.dWo = s.G->W[L]; head.dbo = s.G->b[L];
    head.ldd = ds->ldd; head.Q = d->out_dim; head.d = d->hidden[L - 1];
    head.lam_g = ds->lambda_grad; head.lam_l = ds->lambda_loss; head.loss_sum = s.loss_sum;
    ride.head = &head;
    ride.step_inc = nullptr;
    ride.finish_inc = o->step_dev;
  }
  const bool fin_launch = ks || ds;
  StepOut out;     // where the step's own launches left the squared-norm partials, if they did
  int rc = train_fwd_bwd_impl(s, &ride, &out);
  // (a failure behind the weight-gradient launch: the next batch may be binned, but the caller is not told so and
  //  bins it again)
  if (rc) return rc;
  if (sparse) {
    const bool w0_t = (s.flags & STDADK_FLAG_W0_T) != 0;
    rc = stdadk_sparsity_f32(sparsity, s.P->W[0], s.G->W[0], w0_t ? d->hidden[0] : d->in_dim, w0_t, d->hidden[0],
                             b->p, (int32_t)b->Ks, (int32_t)b->Kt, 1.0f, (float)s.B * (float)d->out_dim, s.loss_sum,
                             nullptr, s.stream);
    if (rc) return rc;
  }
  int n_parts = 0;
  const float *parts = o->sumsq_parts;
  if (clip && out.sq_parts) {
    parts = out.sq_parts; n_parts = out.sq_n;      // partials (and the step advance) came out of the step's launches
  } else if (clip) {
    rc = stdadk_sumsq_f32(o->g, o->n, o->sumsq_parts, fin_launch ? nullptr : o->step_dev, s.stream);
    if (rc) return rc;
    n_parts = STDADK_SUMSQ_PARTS;
  } else if (!fin_launch) {
    rc = stdadk_step_advance(o->step_dev, s.stream);
    if (rc) return rc;
  }
  // with `bin`: the NEXT batch's binning inside this step's optimiser launch (optim.hip: adamw_bin_kernel), when it is
  // the one-launch binning of small batches; the caller then steps on `next_workspace` with STDADK_FLAG_PREBINNED
  const BinSmallArgs *bin = bin_next && !out.binned_next ? &ba : nullptr;
  stdadk_adam_group gr;
  AdamHyper h;
  optim_group(o, clip ? parts : nullptr, n_parts, s.loss_sum, &gr, &h);
  if (ks) {
    // MLP group first: it keeps the guard and the bf16 copies.  The knot group's partials are the finishing launch's.
    stdadk_adam_group kg = *ks->group;
    kg.n_parts = kg.max_norm > 0.f ? STDADK_SUMSQ_PARTS : 0;
    if (!(kg.max_norm > 0.f)) kg.sumsq_parts = nullptr;
    rc = adamw_launch(door, 2, &gr, &kg, h, nullptr, s.stream);
    if (rc == 0 && out.binned_next) *nb.binned = 1;
    return rc;
  }
  rc = adamw_launch("adamw", 1, &gr, nullptr, h, bin, s.stream, (s.flags & STDADK_FLAG_PACK_F32) != 0);
  if (rc == 0 && (bin || out.binned_next)) *nb.binned = 1;
  return rc;
}

extern "C" int stdadk_train_step_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                     const stdadk_mlp_tensors *P, const stdadk_mlp_tensors *G,
                                     const float *coords, const float *t, const float *X, const float *y,
                                     const int64_t *idx, int64_t B, float grad_scale,
                                     const stdadk_loss_desc *loss, const stdadk_sparsity_desc *sparsity,
                                     float *loss_sum, void *workspace, size_t workspace_bytes,
                                     uint64_t drop_seed, int32_t flags, const stdadk_optim_desc *o,
                                     stdadk_stream_t stream) {
  StepCall s = step_call(b, d, P, G, coords, t, X, y, B, grad_scale, loss, loss_sum, workspace, workspace_bytes,
                         drop_seed, flags, stream);
  s.idx = idx;
  return train_step_impl(s, sparsity, o, NextBatch{});
}

extern "C" int stdadk_train_step_next_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                          const stdadk_mlp_tensors *P, const stdadk_mlp_tensors *G,
                                          const float *coords_all, const float *t_all, const float *X_all,
                                          const float *y_all, const int64_t *idx, int64_t B, float grad_scale,
                                          const stdadk_loss_desc *loss, const stdadk_sparsity_desc *sparsity,
                                          float *loss_sum, void *workspace, size_t workspace_bytes,
                                          uint64_t drop_seed, int32_t flags, const stdadk_optim_desc *o,
                                          const int64_t *next_idx, int64_t next_B, int32_t next_y_cols,
                                          void *next_workspace, size_t next_workspace_bytes, int32_t *next_binned,
                                          stdadk_stream_t stream) {
  STDADK_REQUIRE(next_binned, STDADK_E_ARG, "train_step_next: next_binned is NULL");
  StepCall s = step_call(b, d, P, G, coords_all, t_all, X_all, y_all, B, grad_scale, loss, loss_sum, workspace, workspace_bytes,
                         drop_seed, flags, stream);
  s.idx = idx;
  return train_step_impl(s, sparsity, o, {next_idx, next_B, next_y_cols, next_workspace, next_workspace_bytes, next_binned});
}

extern "C" int stdadk_train_step_knots_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                           const stdadk_mlp_tensors *P, const stdadk_mlp_tensors *G,
                                           const float *coords_all, const float *t_all, const float *X_all,
                                           const float *y_all, const int64_t *idx, int64_t B, float grad_scale,
                                           const stdadk_loss_desc *loss, const stdadk_sparsity_desc *sparsity,
                                           float *loss_sum, void *workspace, size_t workspace_bytes,
                                           uint64_t drop_seed, int32_t flags, const stdadk_optim_desc *o,
                                           const int64_t *next_idx, int64_t next_B, int32_t next_y_cols,
                                           void *next_workspace, size_t next_workspace_bytes, int32_t *next_binned,
                                           const stdadk_knot_train *kt, float *d_centers, float *d_log_bw,
                                           const stdadk_adam_group *knots, stdadk_stream_t stream) {
  const bool no_next = !next_idx && next_B == 0 && !next_workspace;
  STDADK_REQUIRE(next_binned || no_next, STDADK_E_ARG, "train_step_knots: next_binned is NULL with a next batch given");
  StepCall s = step_call(b, d, P, G, coords_all, t_all, X_all, y_all, B, grad_scale, loss, loss_sum, workspace, workspace_bytes,
                         drop_seed, flags, stream);
  s.idx = idx;
  KnotStep ks;
  ks.kt = kt; ks.d_centers = d_centers; ks.d_log_bw = d_log_bw; ks.group = knots;
  return train_step_impl(s, sparsity, o, {next_idx, next_B, next_y_cols, next_workspace, next_workspace_bytes, next_binned},
                         &ks);
}

extern "C" int stdadk_train_step_delta_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                           const stdadk_mlp_tensors *P, const stdadk_mlp_tensors *G,
                                           const float *coords_all, const float *t_all, const float *X_all,
                                           const float *y_all, const int64_t *idx, int64_t B, float grad_scale,
                                           const stdadk_loss_desc *loss, const stdadk_sparsity_desc *sparsity,
                                           float *loss_sum, void *workspace, size_t workspace_bytes,
                                           uint64_t drop_seed, int32_t flags, const stdadk_optim_desc *o,
                                           const int64_t *next_idx, int64_t next_B, int32_t next_y_cols,
                                           void *next_workspace, size_t next_workspace_bytes, int32_t *next_binned,
                                           const stdadk_knot_train *kt, float *d_centers, float *d_log_bw,
                                           const stdadk_adam_group *knots, const stdadk_delta_step *head,
                                           stdadk_stream_t stream) {
  const bool no_next = !next_idx && next_B == 0 && !next_workspace;
  STDADK_REQUIRE(next_binned || no_next, STDADK_E_ARG, "train_step_delta: next_binned is NULL with a next batch given");
  STDADK_REQUIRE(head, STDADK_E_ARG, "train_step_delta: head is NULL / incomplete");
  const bool learnable = knots != nullptr;
  STDADK_REQUIRE(learnable ? (d_centers && d_log_bw) : (!kt && !d_centers && !d_log_bw), STDADK_E_ARG,
                 "train_step_delta: kt / d_centers / d_log_bw / knots given in part (all NULL: fixed knots; d_centers, "
                 "d_log_bw and knots all given: learnable knots)");
  StepCall s = step_call(b, d, P, G, coords_all, t_all, X_all, y_all, B, grad_scale, loss, loss_sum, workspace, workspace_bytes,
                         drop_seed, flags, stream);
  s.idx = idx;
  const NextBatch nb = {next_idx, next_B, next_y_cols, next_workspace, next_workspace_bytes, next_binned};
  if (!learnable) return train_step_impl(s, sparsity, o, nb, nullptr, head, "train_step_delta");
  KnotStep ks;
  ks.kt = kt; ks.d_centers = d_centers; ks.d_log_bw = d_log_bw; ks.group = knots;
  return train_step_impl(s, sparsity, o, nb, &ks, head, "train_step_delta");
}

extern "C" int stdadk_bin_batch_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                    const float *coords_all, const float *t_all, const float *X_all,
                                    const float *y_all, const int64_t *idx, int64_t B, int32_t y_cols,
                                    void *workspace, size_t workspace_bytes, int32_t flags,
                                    stdadk_stream_t stream) {
  if (B == 0) return 0;
  Ctx c;
  // (`training` false: this door reads neither dp nor save)
  int rc = open_step(c, b, d, B, workspace, workspace_bytes, flags & ~STDADK_FLAG_PREBINNED, nullptr, nullptr, stream, false);
  if (rc) return rc;
  STDADK_REQUIRE(c.window, STDADK_E_ARG, "bin_batch: only the window path bins its batches");
  STDADK_REQUIRE(coords_all && t_all && (b->p == 0 || X_all), STDADK_E_ARG, "bin_batch: NULL pointer");
  STDADK_REQUIRE(y_cols >= 0 && y_cols <= d->out_dim && (y_cols == 0 || y_all), STDADK_E_ARG,
                 "bin_batch: y_cols=%d must be in 0..Q with y_all given", y_cols);
  BinBuffers bb = plan_bins(c.ws, c.pl);
  // beside a running step the binning goes as several launches of small workgroups, which share CUs
  // with the step's one-workgroup-per-CU kernels; a single 1024-thread workgroup would take a whole CU
  // away from them for its entire duration
  return bin_obs(coords_all, t_all, y_cols > 0 ? y_all : nullptr, y_cols, X_all, b->p, (int)B, c.pl.G, bb,
                 c.st, idx, true);
}

extern "C" int stdadk_train_fwd_bwd_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                        const stdadk_mlp_tensors *P, const stdadk_mlp_tensors *G,
                                        const float *coords, const float *t, const float *X,
                                        const float *y, int64_t B, float grad_scale,
                                        const stdadk_loss_desc *loss, float *loss_sum,
                                        float *y_pred, void *workspace, size_t workspace_bytes,
                                        uint64_t drop_seed, const int32_t *step_dev, int32_t flags,
                                        stdadk_stream_t stream, stdadk_stream_t aux_stream) {
  StepCall s = step_call(b, d, P, G, coords, t, X, y, B, grad_scale, loss, loss_sum, workspace, workspace_bytes,
                         drop_seed, flags, stream);
  s.y_pred = y_pred; s.step_dev = step_dev; s.aux_stream = aux_stream;
  return train_fwd_bwd_impl(s, nullptr, nullptr);
}

extern "C" int stdadk_train_fwd_bwd_indexed_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                                const stdadk_mlp_tensors *P, const stdadk_mlp_tensors *G,
                                                const float *coords_all, const float *t_all,
                                                const float *X_all, const float *y_all, const int64_t *idx,
                                                int64_t B, float grad_scale, const stdadk_loss_desc *loss,
                                                float *loss_sum, float *y_pred, void *workspace,
                                                size_t workspace_bytes, uint64_t drop_seed,
                                                const int32_t *step_dev, int32_t flags,
                                                stdadk_stream_t stream, stdadk_stream_t aux_stream) {
  STDADK_REQUIRE(idx || B == 0, STDADK_E_ARG, "train_fwd_bwd_indexed: idx is NULL");
  StepCall s = step_call(b, d, P, G, coords_all, t_all, X_all, y_all, B, grad_scale, loss, loss_sum, workspace, workspace_bytes,
                         drop_seed, flags, stream);
  s.idx = idx; s.y_pred = y_pred; s.step_dev = step_dev; s.aux_stream = aux_stream;
  return train_fwd_bwd_impl(s, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// validation: indexed forward-only pass + deterministic metrics (eval.hip)
// ---------------------------------------------------------------------------------------------
namespace stdadk {
// the evaluation workspace: [ step plan | metric partials (doubles) | gather buffers of the materialising path ]
struct EvalPlan {
  size_t step_bytes, part, coords, t, y, X, total;     // byte offsets
};
static EvalPlan eval_plan(size_t step_bytes, int64_t B, int Q, int p) {
  EvalPlan e;
  size_t off = align_up(step_bytes, 256);
  e.step_bytes = step_bytes;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes > 0 ? bytes : 1, 256); return o; };
  e.part = take((size_t)EVAL_MAX_WG * EVAL_VALS * sizeof(double));
  e.coords = take((size_t)B * 2 * sizeof(float));
  e.t = take((size_t)B * sizeof(float));
  e.y = take((size_t)B * Q * sizeof(float));
  e.X = take((size_t)B * (p > 0 ? p : 1) * sizeof(float));
  e.total = off;
  return e;
}
}  // namespace stdadk

extern "C" size_t stdadk_eval_workspace_bytes(const stdadk_basis_desc *b, const stdadk_mlp_desc *d, int64_t B,
                                              int32_t flags) {
  const size_t step = stdadk_step_workspace_bytes(b, d, B, flags & ~STDADK_FLAG_PREBINNED);
  if (step == 0) return 0;
  return eval_plan(step, B > 0 ? B : 1, d->out_dim, b->p).total;
}

extern "C" int stdadk_eval_indexed_f32(const stdadk_basis_desc *b, const stdadk_mlp_desc *d,
                                       const stdadk_mlp_tensors *P, const float *coords_all, const float *t_all,
                                       const float *X_all, const float *y_all, const int64_t *idx, int64_t B,
                                       const stdadk_loss_desc *loss, int32_t metric_col, double batch_weight,
                                       double *acc, float *y_pred, void *workspace, size_t workspace_bytes,
                                       int32_t flags, stdadk_stream_t stream) {
  STDADK_REQUIRE(B >= 0, STDADK_E_ARG, "eval_indexed: negative B");
  if (B == 0) return 0;
  STDADK_REQUIRE(!(flags & STDADK_FLAG_PREBINNED), STDADK_E_ARG, "eval_indexed: STDADK_FLAG_PREBINNED is not accepted");
  STDADK_REQUIRE(workspace_bytes >= 256, STDADK_E_WORKSPACE, "eval_indexed: workspace %zu bytes", workspace_bytes);
  Ctx c;
  // the step plan is validated against whatever the workspace holds; the evaluation's own buffers are checked below
  int rc = open_step(c, b, d, B, workspace, workspace_bytes, flags, P, nullptr, stream, false);   // eval mode
  if (rc) return rc;
  const int Q = d->out_dim;
  const EvalPlan ep = eval_plan(c.pl.total_floats * sizeof(float), B, Q, b->p);
  STDADK_REQUIRE(workspace_bytes >= ep.total, STDADK_E_WORKSPACE,
                 "eval_indexed: workspace %zu < %zu bytes (stdadk_eval_workspace_bytes)", workspace_bytes, ep.total);
  STDADK_REQUIRE(P && coords_all && t_all && y_all && idx && acc, STDADK_E_ARG, "eval_indexed: NULL pointer");
  STDADK_REQUIRE(b->p == 0 || X_all, STDADK_E_ARG, "eval_indexed: X_all is NULL with p=%d", b->p);
  STDADK_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7) == 0, STDADK_E_ALIGN, "eval_indexed: acc not 8-byte aligned");
  STDADK_REQUIRE(Q <= STDADK_MAX_Q, STDADK_E_ARG, "eval_indexed: Q=%d above %d", Q, STDADK_MAX_Q);
  STDADK_REQUIRE(metric_col >= 0 && metric_col < Q, STDADK_E_ARG, "eval_indexed: metric_col=%d outside 0..%d",
                 metric_col, Q - 1);
  rc = make_loss(loss, Q, &c.loss);
  if (rc) return rc;
  const LossDev L = c.loss;
  char *base = (char *)workspace;
  double *part = (double *)(base + ep.part);
  if (c.window) {
    // the indexed training step's binning: rows idx[b] read in place, targets carried into sorted order
    c.idx = idx;
    rc = step_forward(c, coords_all, t_all, X_all, y_all, y_pred, nullptr);
    if (rc) return rc;
    return launch_eval_metrics(L, c.ws + c.pl.ypred, c.ws + c.pl.y_s, B, Q, metric_col, batch_weight, part, acc, c.st);
  }
  float *cg = (float *)(base + ep.coords), *tg = (float *)(base + ep.t), *yg = (float *)(base + ep.y);
  float *Xg = b->p > 0 ? (float *)(base + ep.X) : nullptr;
  rc = stdadk_gather_batch_f32(coords_all, t_all, y_all, b->p > 0 ? X_all : nullptr, idx, B, L.y_cols, b->p, cg, tg, yg,
                               Xg, stream);
  if (rc) return rc;
  float *yp = pred_buffer(c, y_pred);
  rc = step_forward(c, cg, tg, Xg, nullptr, yp, nullptr);
  if (rc) return rc;
  return launch_eval_metrics(L, yp, yg, B, Q, metric_col, batch_weight, part, acc, c.st);
}
