// Pieces shared by the bodies of the layer-0 window kernels (l1_body.h: forward, l1_bwd_body.h: per-knot gather of
// dW0^T): the ballot compaction of a pass of candidates, the flat walk over the sorted runs of a rectangle of cells,
// and the XCD-striped order of the knot groups.
#pragma once
#include "window.h"

namespace stdadk {

constexpr int BW_T = 256;        // per-knot gather: 4 waves = 4 knot groups per workgroup

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (lane == 0) ? 0ULL : (~0ULL >> (64 - lane)); }

// Compaction of one pass of 64 candidates into a per-wave list: the lanes that `take` get consecutive places in
// lane order.  pos = this lane's place among them (the list position is the list's fill + pos), m = how many take
// (wave-uniform).  Holds a ballot: every lane of the wave must call it.
struct Compacted { int pos, m; };
__device__ __forceinline__ Compacted compact(bool take, uint64_t below) {
  const uint64_t mask = __ballot(take);
  return {(int)__popcll(mask & below), (int)__popcll(mask)};
}

// Cells [cx_lo, cx_hi] x [cy_lo, cy_hi] of a side x side grid whose members were counting-sorted by cell
// (cs[cx * side + cy] = first sorted position of the cell): a row of cells is one contiguous run of the sorted
// array.  The runs of up to 64 cell rows are fetched by 64 lanes at once and walked as ONE flat candidate list
// (same order as row by row), so ~40 candidates cost two dependent memory round trips instead of two per cell
// row.  visit(position in the sorted array, valid) is called once per pass of 64 candidates on ALL 64 lanes (it
// may hold ballots); the position is meaningless where !valid.
template <class F>
__device__ __forceinline__ void walk_cell_runs(const int *__restrict__ cs, int side, int cx_lo, int cx_hi, int cy_lo,
                                               int cy_hi, int lane, F &&visit) {
  for (int cxb = cx_lo; cxb <= cx_hi; cxb += 64) {
    const int cxl = cxb + lane;
    int seg0 = 0, seg1 = 0;
    if (cxl <= cx_hi) { seg0 = cs[cxl * side + cy_lo]; seg1 = cs[cxl * side + cy_hi + 1]; }
    int incl = seg1 - seg0;                       // inclusive prefix of the run lengths
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    const int total = __shfl(incl, 63, 64);
    for (int f0 = 0; f0 < total; f0 += 64) {
      const int f = f0 + lane;
      // run j with incl[j-1] <= f < incl[j]: first lane whose inclusive prefix exceeds f
      int lo = 0;
#pragma unroll
      for (int st = 32; st > 0; st >>= 1) {
        const int probe = __shfl(incl, lo + st - 1, 64);
        if (probe <= f) lo += st;
      }
      const int jl = lo < 63 ? lo : 63;
      const int pin = __shfl(incl, jl, 64);
      const int pl = __shfl(seg1 - seg0, jl, 64);
      const int ps0 = __shfl(seg0, jl, 64);
      visit(ps0 + (f - (pin - pl)), f < total);
    }
  }
}

// XCD-striped order of the knot groups of the per-knot gather (fixed grid knots, nk = 1 or 2 knots per wave; a group
// is one knot or the pair (ix, iy), (ix, iy + 1)).  Workgroup `block` runs on XCD block & 7 (round-robin dispatch; the
// launch pads the blocks before the knot groups to a multiple of 8).  XCD x owns the grid rows [x side/8, (x+1) side/8)
// of every level: its knots see the observations of one stripe of the domain (+ halo), a contiguous eighth of the
// cell-sorted dZ rows, so each XCD's L2 fetches about 1/5 of dZ_0 instead of all of it.
__host__ __device__ __forceinline__ int knot_groups_per_row(int side, int nk) { return nk == 2 ? (side + 1) >> 1 : side; }
__host__ __device__ __forceinline__ int xcd_first_row(int x, int side) { return (x * side) >> 3; }
__host__ __device__ __forceinline__ int xcd_level_groups(int x, int side, int nk) {
  return (xcd_first_row(x + 1, side) - xcd_first_row(x, side)) * knot_groups_per_row(side, nk);
}

// group of (block, wave): level l (n_levels: the XCD's list is shorter than this slot), first grid row r0 of the XCD on
// that level, index q of the group among the XCD's groups of the level (row by row)
struct XcdGroup { int l, r0, q; };
__device__ __forceinline__ XcdGroup xcd_group_of(const GridView &g, int nk, int block, int wave) {
  const int x = block & 7;
  XcdGroup s = {0, 0, (block >> 3) * (BW_T / 64) + wave};
  for (; s.l < g.n_levels; ++s.l) {
    s.r0 = xcd_first_row(x, g.side[s.l]);
    const int np = xcd_level_groups(x, g.side[s.l], nk);
    if (s.q < np) break;
    s.q -= np;
  }
  return s;
}

}  // namespace stdadk
