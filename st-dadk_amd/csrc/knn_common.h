// What the two exact neighbour searches share (knn.hip: brute force; knn_cells.hip: cell-binned): the KEY of a distance,
// the register list and its insertion, the row as the table holds it, and the argument checks of the common parameter
// list.  Both searches return the k smallest sources in the total order (d2, source index), so they agree bit for bit.
#pragma once
#include "f64_block.h"

namespace stdadk {

typedef unsigned long long u64;

// A distance is carried as its KEY, the bit pattern of the double read as an unsigned integer: d2 is a sum of two
// squares, never negative and never -0, so unsigned order is numeric order, +inf included; every NaN pattern is at or
// above KN_EMPTY (the pattern after +inf's), the key of an empty slot, and `key < last` lets no NaN in.
constexpr u64 KN_EMPTY = 0x7ff0000000000001ull;      // key of an empty slot: above +inf, at or below every NaN
constexpr int KN_NONE = 0x7fffffff;            // index of an empty slot: above every source index
static_assert(STDADK_KNN_MAX_K == 16, "list sizes 1, 2, 4, 8, 16");

// (c, i) into the ascending list: every slot from the first one it is below moves up one, the last falls out.  TOTAL:
// below means (key, index) below; otherwise key strictly below (the caller meets equal keys in index order).
template <int KT, bool TOTAL>
__device__ __forceinline__ void knn_insert(u64 (&key)[KT], int (&ix)[KT], u64 c, int i) {
  bool below[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) below[j] = c < key[j] || (TOTAL && c == key[j] && i < ix[j]);
#pragma unroll
  for (int j = KT - 1; j > 0; --j) {
    key[j] = below[j - 1] ? key[j - 1] : below[j] ? c : key[j];
    ix[j] = below[j - 1] ? ix[j - 1] : below[j] ? i : ix[j];
  }
  key[0] = below[0] ? c : key[0];
  ix[0] = below[0] ? i : ix[0];
}

// slot `at` of the table from a finished list's (key, index)
__device__ __forceinline__ void knn_store_slot(int *nbr_idx, double *nbr_d2, size_t at, u64 key, int ix) {
  const bool none = ix == KN_NONE;
  nbr_idx[at] = none ? -1 : ix;
  nbr_d2[at] = none ? __builtin_inf() : __longlong_as_double((long long)key);
}

static inline bool knn_sizes_ok(int64_t M, int64_t S, int64_t nM, int32_t k) {
  const int64_t lim = 1ll << 31;
  return M >= 0 && S >= 0 && nM >= 0 && M < lim && S < lim && nM < lim && k >= 1 && k <= STDADK_KNN_MAX_K &&
         nM * M < lim && nM * M * k < lim;
}

// The checks of a search's parameter list, in the order the header states them; `need` is the entry's own workspace
// size for these sizes and `sizer` the name of the function that gives it.  0, or the code (the message is set).
static inline int knn_check_call(const char *who, const float *q, int64_t M, const float *coords, int64_t S,
                                 const uint8_t *src, int64_t nM, int32_t k, int32_t exclude_self, int32_t *nbr_idx,
                                 double *nbr_d2, void *workspace, size_t workspace_bytes, size_t need, const char *sizer) {
  const int64_t lim = 1ll << 31;
  STDADK_REQUIRE(M >= 0 && S >= 0 && nM >= 0 && M < lim && S < lim && nM < lim, STDADK_E_ARG,
                 "%s: M=%lld, S=%lld, nM=%lld must be 0 .. 2^31-1", who, (long long)M, (long long)S, (long long)nM);
  STDADK_REQUIRE(k >= 1 && k <= STDADK_KNN_MAX_K, STDADK_E_ARG, "%s: k=%d outside 1..%d", who, k, STDADK_KNN_MAX_K);
  STDADK_REQUIRE(exclude_self == 0 || (exclude_self == 1 && M == S), STDADK_E_ARG,
                 "%s: exclude_self=%d must be 0, or 1 with M == S (M=%lld, S=%lld)", who, exclude_self, (long long)M,
                 (long long)S);
  STDADK_REQUIRE(src || nM == 1 || nM == 0 || S == 0, STDADK_E_ARG,
                 "%s: src == NULL (every site a source) needs nM == 1, got %lld", who, (long long)nM);
  STDADK_REQUIRE(nM * M < lim && nM * M * k < lim, STDADK_E_SHAPE, "%s: nM*M*k = %lld x %lld x %d must stay below 2^31",
                 who, (long long)nM, (long long)M, k);
  const bool rows = M > 0 && nM > 0;
  STDADK_REQUIRE((!rows || (q && nbr_idx && nbr_d2)) && (S == 0 || coords) && workspace, STDADK_E_ARG,
                 "%s: NULL pointer", who);
  STDADK_REQUIRE(((reinterpret_cast<uintptr_t>(nbr_d2)) & 7) == 0, STDADK_E_ALIGN, "%s: nbr_d2 not 8-byte aligned", who);
  STDADK_REQUIRE(((reinterpret_cast<uintptr_t>(nbr_idx) | reinterpret_cast<uintptr_t>(q) |
                   reinterpret_cast<uintptr_t>(coords)) & 3) == 0,
                 STDADK_E_ALIGN, "%s: nbr_idx, q or coords not 4-byte aligned", who);
  if (int rc = check_workspace(who, workspace, workspace_bytes, need, sizer)) return rc;
  const size_t n_out = (size_t)(nM * M) * k;
  const ByteRange out[3] = {{nbr_idx, n_out * sizeof(int32_t)}, {nbr_d2, n_out * sizeof(double)}, {workspace, workspace_bytes}};
  const ByteRange in[3] = {{q, (size_t)M * 2 * sizeof(float)},
                           {coords, (size_t)S * 2 * sizeof(float)},
                           {src, src ? (size_t)nM * S : 0}};
  return check_no_alias(who, out, in, "");
}

}  // namespace stdadk
