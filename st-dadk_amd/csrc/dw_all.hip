// Every weight gradient of a training step that is a reduction over the batch, in ONE launch: the grouped
// split-K products dW_l = dZ_l^T a_(l-1) of the layers after the first (+ the temporal / covariate rows of
// dW0^T) on the matrix cores, and the per-knot gather of the spatial rows of dW0^T.  The two kinds of
// workgroup are independent (both only need the dZ of the backward chain), have the same shape (256
// threads) and complementary bottlenecks (staged MFMA tiles vs L2 row gathers), so sharing the CUs beats
// running them one after the other, and one launch + drain is saved.
#include <stdlib.h>

#include "bin_body.h"
#include "gemm_body.h"
#include "l1_bwd_body.h"

namespace stdadk {

static_assert(GT == BW_T, "the GEMM tiles and the knot groups must share the workgroup shape");
static_assert(GT == BIN_DW_T, "the binning workgroups of the NEXT batch share it too");
// the launch's static LDS block: the staged GEMM tiles, or the binning image (8 KiB more; with the knot bodies' lists
// 35-39 KB per workgroup: the four workgroups per CU that the registers allow fit, 40 KiB each is the limit)
constexpr int DW_ALL_LDS_FLOATS = GROUP_LDS_FLOATS > BIN_DW_LDS_INTS ? GROUP_LDS_FLOATS : BIN_DW_LDS_INTS;

// NK (fixed knots only): 2 neighbouring knots per wave, see l1_window_bwd_multi_body; 1: one knot per wave
// fin.cnt != NULL (FinArgs, gemm_f32.h): the launch also does what the reductions launch behind it did -- block
// order [binning | GEMM tiles | tall reduce jobs | padding | knot groups]
// n_bin > 0: the launch also bins the NEXT batch of the training loop (bin_body.h: bin_dw_body) with n_bin independent
// workgroups that nobody in this launch waits for.  They take the LOWEST block ids: each is one latency chain of
// dependent loads (~10 us) with hardly any bandwidth, so it has to start with the launch to end inside it -- behind
// the GEMM tiles (bin_front == 0, measurement aid STDADK_BIN_POS=mid) the binning workgroups get their CU slots only
// when the first tiles retire and the launch grows by what the optimiser launch saved (27.3 -> 33.1 us; in front
// see DESIGN.md section 6).  The tiles, the tall jobs and the knot groups keep their order and their squared-norm slots.
// -DSTDADK_DIAG builds only (tools/diag/dw_roles.py): the kernel takes a stamp buffer [blocks][16] of wall-clock stamps
// (100 MHz) -- slot 0: role + 1 (0: binning, 1: tall reduce, 10 + j: GEMM job j, 100 + l: knot groups of level l;
// 0 = returned at once), 1 / 2: start / end of the workgroup, 4 + 2w / 5 + 2w: start / end of knot wave w
#ifdef STDADK_DIAG
#define DW_STAMP_PARAM , unsigned long long *stamps
#define DW_STAMP_ARG , stamps
#define DW_STAMP(i, v) do { if (stamps && threadIdx.x == 0) stamps[(size_t)blockIdx.x * 16 + (i)] = (v); } while (0)
#define DW_ROLE(r) DW_STAMP(0, (unsigned long long)(r) + 1)
#define DW_WSTAMP(i) do { if (stamps && (threadIdx.x & 63) == 0) stamps[(size_t)blockIdx.x * 16 + 4 + 2 * (threadIdx.x >> 6) + (i)] = wall_clock64(); } while (0)
#else
#define DW_STAMP_PARAM
#define DW_STAMP_ARG
#define DW_STAMP(i, v) do { } while (0)
#define DW_ROLE(r) do { } while (0)
#define DW_WSTAMP(i) do { } while (0)
#endif
// waves_per_eu(3): a floor of three waves per SIMD for the register allocator.  Without it the kernel took 128 VGPRs +
// 16 AGPRs (the GEMM tile body's budget) = three workgroups per CU, 768 slots for the launch's 784 binning and GEMM
// workgroups, so that no knot group started before the first tiles retired (13 us into a 28 us launch at 4 096 rows,
// profiles/knot_gather_chains.md).  With the floor stated the allocator settles at 98-126 registers and no AGPRs
// (142 for the learnable Wendland body at H = 256, which stays at three), no scratch: FOUR workgroups per CU (the
// static LDS, 35-39 KB, allows four), 1 024 slots, and the first 240 knot workgroups -- the coarse level and a
// quarter of the next -- run beside the tiles from the start.  Same instructions on the same values: bit-identical.
// The attribute is a floor: that the allocator lands at four waves is its choice and may change with the compiler.
// The table of profiles/knot_gather_chains.md is reproduced, and a fall back to three waves seen, with
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage -c dw_all.hip
// ("VGPRs", "AGPRs", "ScratchSize", "Occupancy [waves/SIMD]" per dw_all_kernel instantiation).
template <int CPL, int BASIS, bool KNOTS, int NK>
__global__ __launch_bounds__(GT) __attribute__((amdgpu_waves_per_eu(3)))
void dw_all_kernel(GemmGroup grp, int n_gemm_blocks, L1BwdArgs a, FinArgs fin, ReduceGroup tall, BinSmallArgs bin,
                   int n_bin, int bin_front DW_STAMP_PARAM) {
  __shared__ __attribute__((aligned(16))) float lds[DW_ALL_LDS_FLOATS];
  int blk = (int)blockIdx.x;
  DW_STAMP(1, wall_clock64());
  // (the binning in front is padded to a multiple of 8 blocks: (block & 7), the XCD, stays what the tiles and the knot
  //  groups were laid out for)
  const int lead = bin_front ? (n_bin + 7) & ~7 : 0;          // blockIdx.x = blk + lead
  if (lead) {
    if (blk < n_bin) {
      DW_ROLE(0);
      bin_dw_body(bin, blk, n_bin, reinterpret_cast<int *>(lds));
      DW_STAMP(2, wall_clock64());
      return;
    }
    if (blk < lead) return;
    blk -= lead;
  }
  // GEMM tiles take the low block ids (dispatched first): measured 33.5 us vs 42.5 us the other way round
  if (blk < n_gemm_blocks) {
#ifdef STDADK_DIAG
    { int j = 0; while (j + 1 < grp.n && blk >= grp.first_block[j + 1]) ++j; DW_ROLE(10 + j); }
#endif
    gemm_tn_grouped_block(grp, blk, lds, &fin);
    DW_STAMP(2, wall_clock64());
    return;
  }
  const int n_front = n_gemm_blocks + fin.n_tall;
  if (blk < n_front) {
    DW_ROLE(1);
    const int tb = blk - n_gemm_blocks;
    if (tb == 0 && threadIdx.x == 0 && fin.step_inc) fin.step_inc[0] += 1;
    const float sq = reduce_job_block(tall, tb, lds);
    if (fin.slots) {
      const float t = block4_sum(sq, lds + 256);
      if (threadIdx.x == 0) fin.slots[fin.n_tiles + tb] = t;
    }
    DW_STAMP(2, wall_clock64());
    return;
  }
  const int n_mid = bin_front ? 0 : n_bin;
  if (blk < n_front + n_mid) {
    DW_ROLE(0);
    bin_dw_body(bin, blk - n_front, n_bin, reinterpret_cast<int *>(lds));
    DW_STAMP(2, wall_clock64());
    return;
  }
  // XCD-striped knot groups start at a multiple of 8, so that (group block & 7) is the XCD of the workgroup
  const int first = a.xcd_slots > 0 ? (n_front + n_mid + 7) & ~7 : n_front + n_mid;
  if (blk < first) return;
#ifdef STDADK_DIAG   // (level of the workgroup's first wave; n_levels: an empty slot of a short XCD list)
  if (a.xcd_slots > 0) DW_ROLE(100 + xcd_group_of(a.g, NK, blk - first, 0).l); else DW_ROLE(100);
#endif
  DW_WSTAMP(0);
  float sq;
  if constexpr (NK == 2) sq = l1_window_bwd_multi_body<CPL, BASIS>(a, blk - first);
  else sq = l1_window_bwd_body<CPL, BASIS, KNOTS>(a, blk - first);
  DW_WSTAMP(1);
  if (fin.slots) {                 // workgroup-uniform; every wave of the workgroup arrives (no wave exits early)
    const float t = block4_sum(sq, lds);
    if (threadIdx.x == 0) fin.slots[fin.n_tiles + fin.n_tall + (blk - first)] = t;
  }
  DW_STAMP(2, wall_clock64());
}
#undef DW_STAMP
#undef DW_ROLE
#undef DW_WSTAMP

// kernel arguments travel in the 4 KiB kernarg segment
static_assert(sizeof(GemmGroup) + sizeof(L1BwdArgs) + sizeof(FinArgs) + sizeof(ReduceGroup) + sizeof(BinSmallArgs) + 32 <= 4096,
              "dw_all: kernel arguments exceed the kernarg segment");

int dw_all_knot_blocks(const L1BwdArgs &a) { return knot_plan(a).blocks; }

bool dw_all_bins(int B, int G) { return bin_dw_holds(B, G); }

int launch_dw_all(GemmGroup &grp, const L1BwdArgs &a_in, int basis, hipStream_t st, const FinArgs *fin_in,
                  ReduceGroup *tall_in, int *n_slots, const BinSmallArgs *bin_in) {
  L1BwdArgs a = a_in;
  STDADK_REQUIRE(a.G <= 256, STDADK_E_ARG, "dw_all: G too large");
  STDADK_REQUIRE((int64_t)a.B * a.H < (1ll << 32), STDADK_E_ARG, "dw_all: B*H exceeds 32-bit offsets");
  STDADK_REQUIRE(!a.kpart || a.W0T, STDADK_E_ARG, "dw_all: knot sums need W0^T");
  int ng = 0;
  int rc = gemm_tn_grouped_prepare(grp, &ng);
  if (rc) return rc;
  const KnotPlan kp = knot_plan(a);
  a.xcd_slots = kp.xcd_slots;
  const unsigned n_knot = (unsigned)kp.blocks;
  FinArgs fin;
  ReduceGroup tall;
  if (fin_in && fin_in->cnt) {
    STDADK_REQUIRE(tall_in, STDADK_E_ARG, "dw_all: finishing work without its reduce table");
    fin = *fin_in;
    tall = *tall_in;
    for (int j = 0; j < grp.n; ++j) grp.job[j].coherent_slab = 1;
    fin.n_tall = reduce_jobs_block_count(tall);
    int nt = 0;
    for (int j = 0; j < grp.n; ++j) {
      fin.tile0[j] = nt;
      nt += (int)(ceil_div(grp.job[j].M, 64) * ceil_div(grp.job[j].N, 64));
    }
    STDADK_REQUIRE(nt <= FIN_TILES_MAX, STDADK_E_ARG, "dw_all: %d output tiles (at most %d)", nt, FIN_TILES_MAX);
    fin.n_tiles = nt;
    if (n_slots) *n_slots = nt + fin.n_tall + (int)n_knot;
  } else if (fin_in && fin_in->slots) {      // only the knot workgroups' squared-norm slots
    fin.slots = fin_in->slots;
    if (n_slots) *n_slots = (int)n_knot;
  }
  BinSmallArgs bin{};
  int n_bin = 0, bin_front = 0;
  if (bin_in) {
    STDADK_REQUIRE(bin_dw_holds(bin_in->B, bin_in->G), STDADK_E_ARG,
                   "dw_all: a next batch of %d rows on a grid of %d cells a side does not fit the launch's binning", bin_in->B,
                   bin_in->G);
    bin = *bin_in;
    // (a few hundred rows are not worth splitting: one workgroup)
    n_bin = bin.B >= 1024 ? BIN_DW_WG : 1;
    { const char *e = getenv("STDADK_BIN_WG"); if (e && atoi(e) > 0 && atoi(e) <= 256 && bin.B >= 1024) n_bin = atoi(e); }   // measurement aid
    { const char *e = getenv("STDADK_BIN_POS"); bin_front = (e && e[0] == 'm') ? 0 : 1; }                                     // measurement aid
  }
  // the blocks in front of the knot groups; the knot groups themselves start at a multiple of 8 wherever the binning is
  const unsigned lead = bin_front ? ((unsigned)n_bin + 7u) & ~7u : 0u;
  const unsigned front = (unsigned)ng + (unsigned)fin.n_tall + (bin_front ? 0u : (unsigned)n_bin);
  const unsigned grid = lead + (a.xcd_slots > 0 ? ((front + 7u) & ~7u) : front) + n_knot;
#ifdef STDADK_DIAG
  unsigned long long *stamps = nullptr;
  { const char *e = getenv("STDADK_DW_STAMPS"); if (e) stamps = (unsigned long long *)strtoull(e, nullptr, 0); }
#endif
#define GO(CPL_, BS_)                                                                                      \
  do {                                                                                                     \
    if (a.kpart) STDADK_LAUNCH_NAMED("dw_all_kernel<knots>", (dw_all_kernel<CPL_, BS_, true, 1>),          \
                                     dim3(grid), dim3(GT), 0, st, grp, ng, a, fin, tall, bin, n_bin, bin_front DW_STAMP_ARG); \
    else if (kp.nk == 2) STDADK_LAUNCH_NAMED("dw_all_kernel", (dw_all_kernel<CPL_, BS_, false, 2>), dim3(grid), \
                                             dim3(GT), 0, st, grp, ng, a, fin, tall, bin, n_bin, bin_front DW_STAMP_ARG); \
    else STDADK_LAUNCH_NAMED("dw_all_kernel", (dw_all_kernel<CPL_, BS_, false, 1>), dim3(grid),            \
                             dim3(GT), 0, st, grp, ng, a, fin, tall, bin, n_bin, bin_front DW_STAMP_ARG);               \
  } while (0)
  if (a.H == 256) { if (basis == STDADK_BASIS_WENDLAND) GO(4, 0); else GO(4, 2); }
  else if (a.H == 128) { if (basis == STDADK_BASIS_WENDLAND) GO(2, 0); else GO(2, 2); }
  else { set_error("dw_all: H=%d unsupported", a.H); return STDADK_E_SHAPE; }
#undef GO
#undef DW_STAMP_PARAM
#undef DW_STAMP_ARG
  STDADK_CHECK_LAUNCH("dw_all");
  return 0;
}

}  // namespace stdadk
