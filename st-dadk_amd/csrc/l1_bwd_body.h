// Body of the per-knot gather of dW0^T (see window.h / window.hip), shared by its own kernel and by the
// merged weight-gradient kernel (dw_all.hip).  `block` = index of the group of BW_T/64 knots.
#pragma once
#include "window.h"
#include "basis.h"
#include "l1_body.h"

namespace stdadk {

constexpr int BW_LIST = 64;      // compacted candidates per flush

// d phi / d r as autograd differentiates the forward formulas (compact-support bases of this path)
template <int BASIS>
__device__ __forceinline__ float basis_prime_cs(float r) {
  if (BASIS == STDADK_BASIS_WENDLAND) {
    if (!(r < 1.0f)) return 0.f;
    const float om = 1.0f - r, om2 = om * om;
    return (-56.0f / 3.0f) * r * (om2 * om2 * om) * fmaf(5.0f, r, 1.0f);
  }
  return r <= 1.0f ? -1.0f : 0.f;      // triangular
}

// KNOTS (learnable knots): the wave also accumulates sum_b q_b dZ[b,:] for q = the three per-pair
// factors of d cx, d cy, d log_bw; one dot product with its W0^T row at the end turns them into the
// knot's gradient — sum_b (dZ[b,:] . W0^T[k,:]) q_b without a reduction per pair.
// Returns this lane's share of the squares of the row of dW0^T its wave wrote (0 for a wave without a knot).
template <int CPL, int BASIS, bool KNOTS>
__device__ __forceinline__ float l1_window_bwd_body(const L1BwdArgs &a, const int block) {
  constexpr int H = 64 * CPL;
  constexpr int NQ = KNOTS ? 3 : 0;
  __shared__ float lphi[BW_T / 64][BW_LIST + 8];
  __shared__ int lidx[BW_T / 64][BW_LIST + 8];
  __shared__ float lq[KNOTS ? 3 : 1][BW_T / 64][KNOTS ? BW_LIST + 8 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int k;
  if (a.xcd_slots > 0) {
    const XcdGroup s = xcd_group_of(a.g, 1, block, wave);
    if (s.l >= a.g.n_levels) return 0.f;
    k = a.g.off[s.l] + s.r0 * a.g.side[s.l] + s.q;    // q = (ix - r0) * side + iy
  } else {
    k = block * (BW_T / 64) + wave;                   // knots in table order: level 0 (coarsest) first
    if (k >= a.g.Ks) return 0.f;
  }
  float *my_phi = lphi[wave];
  int *my_idx = lidx[wave];
  const float kcx = a.g.centers[2 * k], kcy = a.g.centers[2 * k + 1];
  const float kbw = a.g.bw[k];
  const float ksc = knot_scale(kbw, a.g.cal);
  const float r = kbw * a.g.cal;                      // support radius
  const int G = a.G;
  // cells overlapping the support square, one cell of margin against rounding
  const int cx_lo = max(floor_clamp((kcx - r) * (float)G, G) - 1, 0);
  const int cx_hi = min(floor_clamp((kcx + r) * (float)G, G) + 1, G - 1);
  const int cy_lo = max(floor_clamp((kcy - r) * (float)G, G) - 1, 0);
  const int cy_hi = min(floor_clamp((kcy + r) * (float)G, G) + 1, G - 1);
  const uint64_t below = lanes_below(lane);

  float acc[CPL];
  float qacc[KNOTS ? 3 : 1][CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    acc[c] = 0.f;
#pragma unroll
    for (int j = 0; j < (KNOTS ? 3 : 1); ++j) qacc[j][c] = 0.f;
  }
  int n = 0;   // entries waiting in the list (wave-uniform)

  auto flush = [&](int cnt) {     // cnt is a multiple of 8
    for (int e0 = 0; e0 < cnt; e0 += 8) {
      float pv[8];
      typename VecT<CPL>::T wv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pv[e] = my_phi[e0 + e];
        wv[e] = *reinterpret_cast<const typename VecT<CPL>::T *>(
            a.dZ + (size_t)((unsigned)my_idx[e0 + e] * (unsigned)H + (unsigned)(CPL * lane)));
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float *f = reinterpret_cast<const float *>(&wv[e]);
#pragma unroll
        for (int c = 0; c < CPL; ++c) acc[c] = fmaf(pv[e], f[c], acc[c]);
        if (KNOTS) {
#pragma unroll
          for (int j = 0; j < NQ; ++j) {
            const float qv = lq[j][wave][e0 + e];
#pragma unroll
            for (int c = 0; c < CPL; ++c) qacc[j][c] = fmaf(qv, f[c], qacc[j][c]);
          }
        }
      }
    }
  };

  walk_cell_runs(a.cell_start, G, cx_lo, cx_hi, cy_lo, cy_hi, lane, [&](int i, bool valid) {
    float phi = 0.f;
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;
    if (valid) {
      if (KNOTS) {
        const float dx = a.xs[i] - kcx, dy = a.ys[i] - kcy;
        const float d = __builtin_amdgcn_sqrtf(fmaf(dx, dx, dy * dy));
        const float rr = d * ksc;
        phi = basis_eval<BASIS>(rr);
        const float gp = basis_prime_cs<BASIS>(rr);
        const float qd = d > 0.f ? gp * ksc / d : 0.f;      // cdist's backward: no pull at zero distance
        q0 = -qd * dx; q1 = -qd * dy; q2 = -gp * rr;
      } else {
        phi = phi_eval<BASIS>(a.xs[i], a.ys[i], kcx, kcy, ksc);
      }
    }
    const Compacted c = compact(phi != 0.f, below);
    if (n + c.m > BW_LIST) {      // not enough room: flush the full groups of 8, keep the remainder
      __builtin_amdgcn_wave_barrier();
      const int full = n & ~7;
      flush(full);
      __builtin_amdgcn_wave_barrier();
      const int rem = n - full;
      float tp = 0.f; int ti = 0;
      float tq[3] = {0.f, 0.f, 0.f};
      if (lane < rem) {
        tp = my_phi[full + lane]; ti = my_idx[full + lane];
        if (KNOTS) { tq[0] = lq[0][wave][full + lane]; tq[1] = lq[1][wave][full + lane]; tq[2] = lq[2][wave][full + lane]; }
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < rem) {
        my_phi[lane] = tp; my_idx[lane] = ti;
        if (KNOTS) { lq[0][wave][lane] = tq[0]; lq[1][wave][lane] = tq[1]; lq[2][wave][lane] = tq[2]; }
      }
      n = rem;
    }
    if (phi != 0.f) {
      const int pos = n + c.pos;
      my_phi[pos] = phi;
      my_idx[pos] = i;
      if (KNOTS) { lq[0][wave][pos] = q0; lq[1][wave][pos] = q1; lq[2][wave][pos] = q2; }
    }
    n += c.m;
  });
  // final flush, zero-padded to a multiple of 8 (row 0 of dZ is a valid address)
  const int npad = (n + 7) & ~7;
  if (lane < npad - n) {
    my_phi[n + lane] = 0.f; my_idx[n + lane] = 0;
    if (KNOTS) { lq[0][wave][n + lane] = 0.f; lq[1][wave][n + lane] = 0.f; lq[2][wave][n + lane] = 0.f; }
  }
  __builtin_amdgcn_wave_barrier();
  flush(npad);
  if (KNOTS) {
    const typename VecT<CPL>::T wk = *reinterpret_cast<const typename VecT<CPL>::T *>(a.W0T + (size_t)(a.g.p + k) * H + CPL * lane);
    const float *wf = reinterpret_cast<const float *>(&wk);
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < CPL; ++c) s = fmaf(qacc[j][c], wf[c], s);
      s = wave_sum(s);
      if (lane == 0) a.kpart[(size_t)j * a.g.Ks + k] = s;
    }
  }

  store_vec<CPL>(a.dW0T + (size_t)(a.g.p + k) * H + CPL * lane, acc);
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < CPL; ++c) sq = fmaf(acc[c], acc[c], sq);
  return sq;
}

// ---------------------------------------------------------------------------------------------------------
// Two neighbouring knots per wave (fixed grid knots): knots (ix, iy), (ix, iy + 1) of a level see almost the same
// observations (supports of 5 spacings, one spacing apart), so the candidates are walked once over the union of the
// supports, a dZ row is fetched once and feeds both accumulators.  Every knot still sums its own non-zero observations
// in sorted order and fmaf(0, dz, acc) == acc, so the rows of dW0^T are bit-identical to the one-knot-per-wave body.
// Groups: level by level, ceil(side / 2) pairs per grid row; the knot past the edge of an odd grid is absent.
// knot_plan() in window.hip counts the groups for the launch.
// Returns this lane's share of the squares of the rows its wave wrote, as l1_window_bwd_body.
template <int CPL, int BASIS>
__device__ __forceinline__ float l1_window_bwd_multi_body(const L1BwdArgs &a, const int block) {
  constexpr int H = 64 * CPL;
  constexpr int NK = 2;
  __shared__ float lphi[BW_T / 64][NK][BW_LIST + 8];
  __shared__ int lidx[BW_T / 64][BW_LIST + 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int l, ix, q;
  if (a.xcd_slots > 0) {
    const XcdGroup s = xcd_group_of(a.g, NK, block, wave);
    l = s.l; ix = s.r0; q = s.q;
  } else {
    l = 0; ix = 0;
    q = block * (BW_T / 64) + wave;                   // group index, level by level
    for (; l < a.g.n_levels; ++l) {
      const int np = a.g.side[l] * knot_groups_per_row(a.g.side[l], NK);
      if (q < np) break;
      q -= np;
    }
  }
  if (l >= a.g.n_levels) return 0.f;
  const int hp = knot_groups_per_row(a.g.side[l], NK);
  ix += q / hp;
  const int iy = 2 * (q % hp);
  const int side = a.g.side[l];
  int kk[NK];
  bool has[NK];
  float kx[NK], ky[NK], ksc[NK];
  float xlo = 3.0e38f, xhi = -3.0e38f, ylo = 3.0e38f, yhi = -3.0e38f;
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    has[j] = iy + j < side;
    kk[j] = a.g.off[l] + ix * side + iy + (has[j] ? j : 0);
    kx[j] = a.g.centers[2 * kk[j]]; ky[j] = a.g.centers[2 * kk[j] + 1];
    const float bw = a.g.bw[kk[j]];
    ksc[j] = knot_scale(bw, a.g.cal);
    const float r = bw * a.g.cal;                     // support radius
    xlo = fminf(xlo, kx[j] - r); xhi = fmaxf(xhi, kx[j] + r);
    ylo = fminf(ylo, ky[j] - r); yhi = fmaxf(yhi, ky[j] + r);
  }
  int *my_idx = lidx[wave];
  const int G = a.G;
  // cells overlapping any of the support squares, one cell of margin against rounding
  const int cx_lo = max(floor_clamp(xlo * (float)G, G) - 1, 0);
  const int cx_hi = min(floor_clamp(xhi * (float)G, G) + 1, G - 1);
  const int cy_lo = max(floor_clamp(ylo * (float)G, G) - 1, 0);
  const int cy_hi = min(floor_clamp(yhi * (float)G, G) + 1, G - 1);
  const uint64_t below = lanes_below(lane);

  float acc[NK][CPL];
#pragma unroll
  for (int j = 0; j < NK; ++j)
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[j][c] = 0.f;
  int n = 0;

  auto flush = [&](int cnt) {     // cnt is a multiple of 8
    for (int e0 = 0; e0 < cnt; e0 += 8) {
      typename VecT<CPL>::T wv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        wv[e] = *reinterpret_cast<const typename VecT<CPL>::T *>(
            a.dZ + (size_t)((unsigned)my_idx[e0 + e] * (unsigned)H + (unsigned)(CPL * lane)));
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float *f = reinterpret_cast<const float *>(&wv[e]);
#pragma unroll
        for (int j = 0; j < NK; ++j) {
          const float pv = lphi[wave][j][e0 + e];
#pragma unroll
          for (int c = 0; c < CPL; ++c) acc[j][c] = fmaf(pv, f[c], acc[j][c]);
        }
      }
    }
  };

  walk_cell_runs(a.cell_start, G, cx_lo, cx_hi, cy_lo, cy_hi, lane, [&](int i, bool valid) {
    float pv[NK];
    bool any = false;
#pragma unroll
    for (int j = 0; j < NK; ++j) pv[j] = 0.f;
    if (valid) {
      const float x = a.xs[i], y = a.ys[i];
#pragma unroll
      for (int j = 0; j < NK; ++j) {
        pv[j] = has[j] ? phi_eval<BASIS>(x, y, kx[j], ky[j], ksc[j]) : 0.f;
        any = any || pv[j] != 0.f;
      }
    }
    const Compacted c = compact(any, below);
    if (n + c.m > BW_LIST) {      // not enough room: flush the full groups of 8, keep the remainder
      __builtin_amdgcn_wave_barrier();
      const int full = n & ~7;
      flush(full);
      __builtin_amdgcn_wave_barrier();
      const int rem = n - full;
      float tp[NK]; int ti = 0;
#pragma unroll
      for (int j = 0; j < NK; ++j) tp[j] = 0.f;
      if (lane < rem) {
#pragma unroll
        for (int j = 0; j < NK; ++j) tp[j] = lphi[wave][j][full + lane];
        ti = my_idx[full + lane];
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < rem) {
#pragma unroll
        for (int j = 0; j < NK; ++j) lphi[wave][j][lane] = tp[j];
        my_idx[lane] = ti;
      }
      n = rem;
    }
    if (any) {
      const int pos = n + c.pos;
#pragma unroll
      for (int j = 0; j < NK; ++j) lphi[wave][j][pos] = pv[j];
      my_idx[pos] = i;
    }
    n += c.m;
  });
  const int npad = (n + 7) & ~7;
  if (lane < npad - n) {
#pragma unroll
    for (int j = 0; j < NK; ++j) lphi[wave][j][n + lane] = 0.f;
    my_idx[n + lane] = 0;
  }
  __builtin_amdgcn_wave_barrier();
  flush(npad);

  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    if (has[j]) {
#pragma unroll
      for (int c = 0; c < CPL; ++c) sq = fmaf(acc[j][c], acc[j][c], sq);
      store_vec<CPL>(a.dW0T + (size_t)(a.g.p + kk[j]) * H + CPL * lane, acc[j]);
    }
  }
  return sq;
}

}  // namespace stdadk
