// Host sanitizer coverage of the two conformal entry points without Python: a stand-alone program that drives the
// argument checks and the planning of stdadk_conformal_scores_f32 and stdadk_select_f32 under STDADK_DRY_RUN=1 (no HIP
// call is made, so it runs without a GPU).  Build and run from st-dadk_amd/csrc (ROCm's hipcc):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -x hip api.cpp conformal.hip ../../tools/conformal_args_main.cpp \
//         -o conformal_args && STDADK_DRY_RUN=1 ./conformal_args
// Exit status 0 and "conformal args: N calls" = every call returned the expected code and the sanitizers saw nothing.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/stdadk.h"

static int g_calls = 0, g_bad = 0;
static void expect(int rc, int want, const char *what) {
  ++g_calls;
  if (rc != want) {
    ++g_bad;
    fprintf(stderr, "%s: rc=%d, expected %d (%s)\n", what, rc, want, stdadk_last_error());
  }
}

int main() {
  const char *dry = getenv("STDADK_DRY_RUN");
  if (!dry || strcmp(dry, "1") != 0) {
    fprintf(stderr, "run with STDADK_DRY_RUN=1: this program must not launch\n");
    return 2;
  }
  // one honest host buffer stands behind every device pointer: the host code never dereferences them
  static double buf[1 << 13];
  char *base = (char *)buf;
  float *f = (float *)base;
  int64_t *i64 = (int64_t *)base;
  int32_t *i32 = (int32_t *)base;
  const size_t ws_scores = stdadk_conformal_scores_workspace_bytes(100, 3), ws_sel = stdadk_select_workspace_bytes(2);

  // ---- scores: arrays sized exactly C x 3 and G, so an index past them is a report
  int32_t *cols = (int32_t *)malloc(2 * 3 * sizeof(int32_t)), *codes = (int32_t *)malloc(2 * sizeof(int32_t));
  const int32_t honest[6] = {STDADK_CONFORMAL_RESID, 0, 0, STDADK_CONFORMAL_CQR, 0, 2};
  memcpy(cols, honest, sizeof honest);
  codes[0] = 2; codes[1] = 3;
#define SCORES(S, nT, Q, C, G, cap, count, ws, wsb) \
  stdadk_conformal_scores_f32(f, f, nullptr, S, nT, Q, cols, C, codes, G, f, cap, count, i32, ws, wsb, nullptr)
  expect(SCORES(100, 3, 3, 2, 2, 50, i64, base, ws_scores), 0, "scores ok");
  expect(SCORES(0, 3, 3, 2, 2, 50, i64, nullptr, 0), 0, "scores empty");
  expect(SCORES(-1, 3, 3, 2, 2, 50, i64, base, ws_scores), STDADK_E_ARG, "scores S<0");
  expect(SCORES(100, 3, 9, 2, 2, 50, i64, base, ws_scores), STDADK_E_ARG, "scores Q");
  expect(SCORES(100, 3, 3, 9, 2, 50, i64, base, ws_scores), STDADK_E_ARG, "scores C");
  expect(SCORES(100, 3, 3, 2, 3, 50, i64, base, ws_scores), STDADK_E_ARG, "scores G");
  expect(SCORES(100, 3, 2, 2, 2, 50, i64, base, ws_scores), STDADK_E_ARG, "scores col_b >= Q");
  expect(SCORES(100, 3, 3, 2, 2, -1, i64, base, ws_scores), STDADK_E_ARG, "scores cap<0");
  expect(SCORES(1 << 20, 1 << 12, 3, 2, 2, 50, i64, base, ws_scores), STDADK_E_SHAPE, "scores rows");
  expect(SCORES(100, 3, 3, 2, 2, 1ll << 31, i64, base, ws_scores), STDADK_E_SHAPE, "scores cap");
  expect(SCORES(100, 3, 3, 2, 2, 50, (int64_t *)(base + 4), base, ws_scores), STDADK_E_ALIGN, "scores count align");
  expect(SCORES(100, 3, 3, 2, 2, 50, i64, base + 4, ws_scores), STDADK_E_ALIGN, "scores ws align");
  expect(SCORES(100, 3, 3, 2, 2, 50, i64, base, ws_scores - 8), STDADK_E_WORKSPACE, "scores ws small");
  cols[0] = 3;
  expect(SCORES(100, 3, 3, 2, 2, 50, i64, base, ws_scores), STDADK_E_ARG, "scores kind");
  cols[0] = STDADK_CONFORMAL_ABS; codes[1] = 256;
  expect(SCORES(100, 3, 3, 2, 2, 50, i64, base, ws_scores), STDADK_E_ARG, "scores code");
  free(cols); free(codes);

  // ---- select: every count of selections with arrays of exactly that length
  for (int n_sel = 1; n_sel <= STDADK_SELECT_MAX; ++n_sel) {
    int32_t *sc = (int32_t *)malloc(n_sel * sizeof(int32_t));
    int64_t *sr = (int64_t *)malloc(n_sel * sizeof(int64_t));
    double *sb = (double *)malloc(n_sel * sizeof(double));
    for (int j = 0; j < n_sel; ++j) {
      sc[j] = (j * 3) % 8; sr[j] = j % 2 ? -1 : j; sb[j] = j / 16.0;
    }
    expect(stdadk_select_f32(f, 100, 8, i64, 100, sc, sr, sb, n_sel, f, i64, base, stdadk_select_workspace_bytes(n_sel),
                             nullptr), 0, "select ok");
    sc[n_sel - 1] = 8;
    expect(stdadk_select_f32(f, 100, 8, i64, 100, sc, sr, sb, n_sel, f, i64, base, ws_sel, nullptr), STDADK_E_ARG,
           "select column");
    free(sc); free(sr); free(sb);
  }
  int32_t sc[2] = {0, 1};
  int64_t sr[2] = {0, -1};
  double sb[2] = {0.0, 0.9};
#define SELECT(stride, C, n, n_max, betas, n_sel, ws, wsb) \
  stdadk_select_f32(f, stride, C, n, n_max, sc, sr, betas, n_sel, f, i64, ws, wsb, nullptr)
  expect(SELECT(100, 2, i64, 100, sb, 2, base, ws_sel), 0, "select ok 2");
  expect(SELECT(100, 2, i64, 0, sb, 2, base, ws_sel), 0, "select n_max 0");
  expect(SELECT(100, 2, i64, 100, sb, 0, base, ws_sel), STDADK_E_ARG, "select n_sel 0");
  expect(SELECT(100, 2, i64, 100, sb, 17, base, ws_sel), STDADK_E_ARG, "select n_sel 17");
  expect(SELECT(100, 9, i64, 100, sb, 2, base, ws_sel), STDADK_E_ARG, "select C");
  expect(SELECT(100, 2, i64, 100, nullptr, 2, base, ws_sel), STDADK_E_ARG, "select no beta");
  expect(SELECT(100, 2, nullptr, 100, sb, 2, base, ws_sel), STDADK_E_ARG, "select n NULL");
  expect(SELECT(100, 2, i64, -1, sb, 2, base, ws_sel), STDADK_E_ARG, "select n_max<0");
  expect(SELECT(99, 2, i64, 100, sb, 2, base, ws_sel), STDADK_E_SHAPE, "select stride");
  expect(SELECT(1ll << 31, 2, i64, 1ll << 31, sb, 2, base, ws_sel), STDADK_E_SHAPE, "select n_max 2^31");
  expect(SELECT(100, 2, (int64_t *)(base + 4), 100, sb, 2, base, ws_sel), STDADK_E_ALIGN, "select n align");
  expect(SELECT(100, 2, i64, 100, sb, 2, base + 4, ws_sel), STDADK_E_ALIGN, "select ws align");
  expect(SELECT(100, 2, i64, 100, sb, 2, base, ws_sel - 8), STDADK_E_WORKSPACE, "select ws small");
  sb[1] = 1.5;
  expect(SELECT(100, 2, i64, 100, sb, 2, base, ws_sel), STDADK_E_ARG, "select beta > 1");
  printf("conformal args: %d calls, %d unexpected\n", g_calls, g_bad);
  return g_bad ? 1 : 0;
}
