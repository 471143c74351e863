/*
 * stdadk.h — C ABI of libstdadk.so, the MI355X (gfx950) implementation of ST-DADK's
 * spatio-temporal interpolation hot path.
 *
 * The reference (STLABTW/ST-DADK) is pure Python on PyTorch and has no FFI layer; the boundary its
 * driver sees is the nn.Module surface of stnf/models/st_interp.py.  Each entry point below names
 * the reference function (file:line, relative to the reference root) whose arithmetic it replaces.
 * The Python face (st-dadk_amd/stnf) binds these symbols with ctypes; INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer (hipMalloc / torch
 *     allocator) unless the parameter says "host".  Inputs are borrowed, outputs are written into
 *     caller-provided buffers; the library allocates nothing and keeps no global mutable state.
 *   - `stream` is a hipStream_t (0 = default stream).  Every call only enqueues work on it:
 *     no host<->device sync, no host read of device scalars => hipGraph-capturable.
 *   - all matrices are row-major fp32; `ld*` is the row stride in elements.
 *   - return value: 0 on success; <0 argument error (STDADK_E_*); >0 a hipError_t.
 *     stdadk_last_error() returns a thread-local message for the last non-zero return.
 */
#ifndef STDADK_H
#define STDADK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STDADK_ABI_VERSION 10
#define STDADK_MAX_HIDDEN 8
#define STDADK_MAX_LEVELS 8
#define STDADK_SUMSQ_PARTS 256 /* partial sums written by stdadk_sumsq_f32 */

#define STDADK_E_ARG (-1)     /* null pointer / negative size / bad enum       */
#define STDADK_E_SHAPE (-2)   /* shapes inconsistent with the descriptor      */
#define STDADK_E_ALIGN (-3)   /* buffer not aligned as documented             */
#define STDADK_E_WORKSPACE (-4) /* workspace smaller than *_workspace_bytes() */

typedef void *stdadk_stream_t; /* hipStream_t */

/* SpatialBasisEmbedding.basis_function, stnf/models/st_interp.py:56-60,451-458 */
enum { STDADK_BASIS_WENDLAND = 0, STDADK_BASIS_GAUSSIAN = 1, STDADK_BASIS_TRIANGULAR = 2 };

int stdadk_abi_version(void);
const char *stdadk_last_error(void);

/* ------------------------------------------------------------------------------------------
 * A2-A5  feature builder (materialising):  out[b, :] = [ X[b, 0:p] | phi(coords[b]) | psi(t[b]) ]
 *
 * Replaces SpatialBasisEmbedding.forward + _wendland/_gaussian/_triangular
 * (stnf/models/st_interp.py:433-491), TemporalBasisEmbedding.forward (:583-596) and the
 * torch.cat of STInterpMLP.forward (:843-846).
 *   phi[b,k] = f( sqrt((x-cx_k)^2+(y-cy_k)^2) / (bw_k * cal) ),  cal = 1 / 0.223477 / 0.654714
 *   psi[b,j] = exp(-0.5 * ((t-c_j)/bw_j)^2)
 * coords [B,2], t [B] (the reference's (B,1) column), X [B,p] or NULL when p == 0,
 * s_centers [Ks,2], s_bw [Ks], t_centers [Kt], t_bw [Kt]; Ks or Kt may be 0.
 * out [B, ld_out], ld_out >= p+Ks+Kt; columns beyond p+Ks+Kt (row padding) are zero-filled.
 * ------------------------------------------------------------------------------------------ */
int stdadk_rbf_build_f32(const float *coords, const float *t, const float *X, int64_t B, int32_t p,
                         const float *s_centers, const float *s_bw, int64_t Ks, int32_t basis,
                         const float *t_centers, const float *t_bw, int64_t Kt, float *out,
                         int64_t ld_out, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A6  MLP  (Linear -> LayerNorm -> ReLU -> Dropout) x L -> Linear      st_interp.py:656-690,880
 * ------------------------------------------------------------------------------------------ */
typedef struct stdadk_mlp_desc {
  int32_t n_hidden;                  /* L, 0..STDADK_MAX_HIDDEN                               */
  int32_t in_dim;                    /* D = p + Ks + Kt                                       */
  int32_t hidden[STDADK_MAX_HIDDEN]; /* hidden_dims                                           */
  int32_t out_dim;                   /* Q (1 for MSE regression)                              */
  int32_t layernorm;                 /* 0/1; eps below (nn.LayerNorm default 1e-5)            */
  float ln_eps;
  float dropout_p;                   /* 0 => no dropout layers                                */
} stdadk_mlp_desc;

/* Device pointers of the parameters / their gradients; layer l = 0..L-1 are the hidden Linear
 * (+LayerNorm) layers, layer L is the output Linear.  W[l] is (out,in) row-major contiguous as
 * nn.Linear stores it; ln_g/ln_b are NULL when layernorm == 0.
 * W_bf16 / WT_bf16 (parameters only, read with STDADK_FLAG_BF16; NULL otherwise): bfloat16 copies of the
 * hidden layers l >= 1 -- W_bf16[l] is W[l] rounded to nearest-even, (out,in) row-major; WT_bf16[l] its
 * transpose (in,out) row-major (the K-contiguous operand of dA = dZ W).  stdadk_bf16_shadow_refresh makes
 * them, the optimiser entry points keep them current (stdadk_bf16_shadow).
 * With STDADK_FLAG_PACK_F32 the same slots are read as `float *`: W_bf16[l] is the packed forward copy PF
 * and WT_bf16[l] the packed backward copy PB of W[l], l = 1 .. L-1 (layout below, at stdadk_f32_pack_refresh). */
typedef struct stdadk_mlp_tensors {
  float *W[STDADK_MAX_HIDDEN + 1];
  float *b[STDADK_MAX_HIDDEN + 1];
  float *ln_g[STDADK_MAX_HIDDEN];
  float *ln_b[STDADK_MAX_HIDDEN];
  uint16_t *W_bf16[STDADK_MAX_HIDDEN + 1];
  uint16_t *WT_bf16[STDADK_MAX_HIDDEN + 1];
} stdadk_mlp_tensors;

/* Bytes of workspace stdadk_mlp_forward_f32/backward_f32 need for B rows (saved activations +
 * split-K slabs).  The same workspace must be passed to backward untouched. */
size_t stdadk_mlp_workspace_bytes(const stdadk_mlp_desc *desc, int64_t B);

/* Dropout keep-masks: "the counter-based generator keyed by drop_seed", everywhere below.  Stateless:
 * the keep decision of element (row, col) of hidden layer `layer` (0-based) is a pure function of
 * (drop_seed, step, layer, row, col), so a backward regenerates the mask of its forward.
 *   step seed  s = drop_seed + step_dev[0] * 0x9E3779B97F4A7C15  mod 2^64   (step_dev NULL: s = drop_seed)
 *   row key    k = mix32(s ^ (0x9E3779B97F4A7C15 * (layer + 1) mod 2^64) ^ (row * 0xD1B54A32D192ED03 mod 2^64))
 *              mix32(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53;
 *                        x ^= x >> 33 (64-bit, wrapping); the low 32 bits
 *   hash       h = fin32(k ^ (pair * 0x9E3779B1 mod 2^32)),  pair = (col & 63) | ((col >> 7) << 6): the columns
 *              c and c + 64 of a 128-column block share one hash
 *              fin32(h): h ^= h >> 16; h *= 0x21f0aaad; h ^= h >> 15; h *= 0x735a2d97; h ^= h >> 15 (32-bit)
 *   bits       v = bit 6 of col set ? h >> 16 : h & 0xffff
 *   keep       v >= ceilf(p * 65536) with p = dropout_p as float32; kept values are scaled by 1 / (1 - p)
 * `row` is the caller's row wherever the features are materialised (stdadk_mlp_*_f32, and the step entry
 * points on the materialising path).  On the window path it is the row's SORTED position: the batch is
 * sorted by binning-cell key (stable: ascending caller row inside a cell) on the grid of
 * pick_cell_grid(B) cells a side, the smallest power of two in [8, 256] whose square is >= B.
 * step_dev[0]: forward and backward of one step read the value the counter has BEFORE that step's own
 * advance, which rides behind the backward (with the clip-norm partial sums, or stdadk_step_advance);
 * the optimiser launch reads the advanced value.  The n-th step since the counter was zeroed (n from 0)
 * therefore draws the masks of step n, in eager launches and in a replayed graph alike.
 * oracle/dropout.py restates this on the CPU for the tests. */

/* y_pred[B,Q] = mlp(features[B, ldf]).  `training` != 0 applies dropout (keep-mask from the
 * counter-based generator keyed by drop_seed, or from drop_mask[l] (uint8 [B,h_l], 1 = keep) when
 * that host array of device pointers is non-NULL) and saves what backward needs in `workspace`. */
int stdadk_mlp_forward_f32(const stdadk_mlp_desc *desc, const stdadk_mlp_tensors *params,
                           const float *features, int64_t ldf, int64_t B, float *y_pred,
                           void *workspace, size_t workspace_bytes, int32_t training,
                           uint64_t drop_seed, const uint8_t *const *drop_mask,
                           stdadk_stream_t stream);

/* A8  loss.backward() through A6 (scripts/train_st_interp.py:693): given dY[B,Q] = dLoss/dy_pred,
 * writes every parameter gradient into `grads` (overwrite, not accumulate).  Knots are buffers in
 * the fixed-basis model, so no gradient flows into the features and dX of layer 0 is skipped. */
int stdadk_mlp_backward_f32(const stdadk_mlp_desc *desc, const stdadk_mlp_tensors *params,
                            const stdadk_mlp_tensors *grads, const float *features, int64_t ldf,
                            int64_t B, const float *dY, void *workspace, size_t workspace_bytes,
                            uint64_t drop_seed, const uint8_t *const *drop_mask,
                            stdadk_stream_t stream);

/* A7  nn.MSELoss() (scripts/train_st_interp.py:549,621) fused with its gradient:
 *   loss_sum[0] += sum((y_pred-y)^2)   (caller divides by the global element count)
 *   dY[i] = 2*(y_pred[i]-y[i])*grad_scale          (grad_scale = 1/(B*Q) for the plain mean)
 * n = B*Q elements.  dY may be NULL (evaluation); loss_sum may be NULL. */
int stdadk_mse_f32(const float *y_pred, const float *y, int64_t n, float grad_scale, float *dY,
                   float *loss_sum, stdadk_stream_t stream);

/* N3  quantile / multi-quantile objectives (scripts/train_st_interp.py:37-88,622-658) fused with
 * their gradient, as a generalisation of stdadk_mse_f32.  For y_pred [B,Q] and y [B,y_cols]:
 *   STDADK_LOSS_MSE     : sum (y_pred - y)^2
 *   STDADK_LOSS_PINBALL : sum_q sum_b max((tau_q-1) e, tau_q e), e = y - y_pred   (quantile_loss, :37-50;
 *                         the multi-quantile mean over q of per-quantile means, :625-632, is this sum
 *                         divided by B*Q), plus the prediction-level non-crossing penalty
 *                         nc_weight * mean_b sum_k relu(y_pred[b,k] - y_pred[b,k+1])^nc_power
 *                         (non_crossing_penalty, :53-88, reduction "mean"; added as nc_weight*Q*sum so
 *                         that loss_sum / (B*Q) is the reference's batch loss).
 *   loss_sum[0] += that sum;   dY = grad_scale * d(sum)/dy_pred     (grad_scale = 1/(B*Q) for the mean)
 * Sub-gradients follow torch: max() splits ties 1/2:1/2, relu'(0) = 0.  y_cols == 1 broadcasts one
 * target over the Q outputs (the (B,1) targets of multi-quantile training). */
#define STDADK_LOSS_MSE 0
#define STDADK_LOSS_PINBALL 1
#define STDADK_MAX_Q 8
typedef struct stdadk_loss_desc {
  int32_t kind;             /* STDADK_LOSS_*                                                    */
  int32_t y_cols;           /* columns of y: Q, or 1 (broadcast)                                */
  float tau[STDADK_MAX_Q];  /* quantile levels of the Q outputs (PINBALL)                       */
  float nc_weight;          /* prediction-level non-crossing weight, 0 = off (PINBALL, Q > 1)   */
  int32_t nc_power;         /* 1 (hinge) or 2 (squared hinge)                                   */
} stdadk_loss_desc;
int stdadk_loss_f32(const stdadk_loss_desc *loss, const float *y_pred, const float *y, int64_t B,
                    int32_t Q, float grad_scale, float *dY, float *loss_sum, stdadk_stream_t stream);

/* N3  delta-reparameterised output head (stnf/models/st_interp.py:671-686,849-877): the Q output
 * rows are cumulative sums of per-quantile vectors delta_k = (delta_k0 | delta_k1..d),
 *   beta_k = sum_{l<=k} delta_l,   Wo[k,:] = beta_k[1:],  bo[k] = beta_k[0],
 * so the step-level entry points run unchanged on (Wo, bo).  delta is [Q, ldd] (ldd >= d+1).
 * stdadk_delta_head_f32 builds Wo [Q,d] and bo [Q]; stdadk_delta_head_backward_f32 maps (dWo, dbo)
 * back, d_delta_l = sum_{k>=l} d beta_k (overwrite), and adds the parameter-level penalty of
 * compute_p_nc_delta_penalty (scripts/train_st_interp.py:91-160, used at :640-649):
 *   P = sum_{k>=2} (delta_k0 - max(delta_k0, S_k)),  S_k = sum_j max(0, -delta_kj)
 *   d_delta += lambda_grad * dP/d delta;   loss_sum[0] += lambda_loss * P   (loss_sum may be NULL)
 * with torch's sub-gradients (max ties 1/2:1/2, clamp(min=0) passes the gradient at 0). */
int stdadk_delta_head_f32(const float *delta, int64_t ldd, int32_t Q, int32_t d, float *Wo,
                          float *bo, stdadk_stream_t stream);
int stdadk_delta_head_backward_f32(const float *delta, const float *dWo, const float *dbo,
                                   int64_t ldd, int32_t Q, int32_t d, float lambda_grad,
                                   float lambda_loss, float *d_delta, float *loss_sum,
                                   stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A9  clip_grad_norm_ + AdamW + EMA on flat fp32 buffers of n elements
 * (scripts/train_st_interp.py:696-712, stnf/utils/ema.py:52-66, torch.optim.AdamW).
 *   stdadk_sumsq_f32 : parts[0..STDADK_SUMSQ_PARTS) = partial sums of g^2 (all entries written, fixed
 *                      order => reproducible; several tensors may each fill their own block of
 *                      partials).  After an all-reduce of the gradients this gives the post-reduce
 *                      global norm the clip must use.
 *   stdadk_adamw_ema_f32: ss = sum(sumsq_parts[0..n_parts));
 *       coef = min(1, max_norm/(sqrt(ss)+1e-6)) if max_norm > 0 else 1
 *       g' = g*coef*grad_mul; p *= 1-lr*wd; m = b1*m+(1-b1)*g'; v = b2*v+(1-b2)*g'^2;
 *       p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps);
 *       ema = decay*ema + (1-decay)*p   (skipped when ema == NULL)
 *   lr is read from the device scalar lr_dev[0] when non-NULL (graph-replayable schedules),
 *   else from `lr`.  The 1-based number of the step being applied is `step` (host value) or, when
 *   step_dev is non-NULL, the device scalar step_dev[0].  That counter also feeds the dropout
 *   generator (as "steps completed") in the forward/backward of a step, so it must be advanced
 *   AFTER the backward and BEFORE stdadk_adamw_ema_f32: pass it as `step_inc` to
 *   stdadk_sumsq_f32 (block 0 adds 1) or call stdadk_step_advance when no clipping is used.
 * ------------------------------------------------------------------------------------------ */
int stdadk_sumsq_f32(const float *g, int64_t n, float *parts, int32_t *step_inc,
                     stdadk_stream_t stream);

/* BASELINE config C3 ("bf16 MLP with MFMA"): fp32 MASTER weights, bf16 OPERAND copies.  A shadow table names
 * up to STDADK_MAX_HIDDEN regions of a flat fp32 parameter buffer, each a (rows, cols) row-major matrix at
 * element offset `off` (off and cols multiples of 4), with the bf16 copy `dst` [rows][cols] and its transpose
 * `dst_t` [cols][rows] (either may be NULL).  stdadk_bf16_shadow_refresh rewrites every region from p (after
 * load_state_dict, an EMA swap, ...); the optimiser entry points below take the table as an optional last
 * argument and rewrite the copies from the values they have just stepped, in the same pass (offsets relative
 * to the `p` of that call).  Rounding: round-to-nearest-even (v_cvt_pk_bf16_f32). */
typedef struct stdadk_bf16_region {
  int64_t off;          /* first element of the matrix in the flat buffer                     */
  int32_t rows, cols;
  uint16_t *dst;        /* [rows][cols] bf16 or NULL                                          */
  uint16_t *dst_t;      /* [cols][rows] bf16 or NULL                                          */
} stdadk_bf16_region;
typedef struct stdadk_bf16_shadow {
  int32_t n;                                     /* regions in use                            */
  stdadk_bf16_region r[STDADK_MAX_HIDDEN];
} stdadk_bf16_shadow;
int stdadk_bf16_shadow_refresh(const float *p, const stdadk_bf16_shadow *shadow, stdadk_stream_t stream);

/* Fragment-order fp32 copies of the hidden weights (STDADK_FLAG_PACK_F32; an addition within ABI 10:
 * one new entry point and one new flag bit, no struct, signature or default behaviour changed).  The fused tail kernels give every
 * lane of a wave, per 32-deep K chunk c of its 16-column N tile nt, two float4 of weights (halves j = 0, 1); a packed
 * copy stores those float4 in the order they are loaded, so that a wave's load is one contiguous KiB.  For a hidden
 * layer l >= 1 (not the output head) with W = W[l] (rows = out, cols = in) row-major, lane = 16 q + c16 (q = 0..3,
 * c16 = 0..15) and e = 0..3, chunk-major over all N tiles, entries with k beyond K zero:
 *   forward copy PF (z = a W^T):  N = rows, K = cols, NT = N/16, NCH = ceil(K/32)
 *     PF[(((c NT + nt) 2 + j) 64 + lane) 4 + e] = W[16 nt + c16][32 c + 16 j + 4 q + e]
 *   backward copy PB (dA = dZ W): K = rows, N = cols, NT = cols/16, NCH = ceil(rows/32)
 *     PB[(((c NT + nt) 2 + j) 64 + lane) 4 + e] = W[32 c + 16 j + 4 q + e][16 nt + c16]
 * Each copy holds NCH * NT * 512 floats (PF: 32 rows ceil(cols/32), PB: 32 cols ceil(rows/32)), is owned by the caller
 * and must be 16-byte aligned (STDADK_E_ALIGN); rows and cols are multiples of 16 (STDADK_E_SHAPE).  The table is a
 * stdadk_bf16_shadow whose `dst` / `dst_t` are reinterpreted: `dst` = (float *) PF, `dst_t` = (float *) PB (either may
 * be NULL).  stdadk_f32_pack_refresh rebuilds every region's copies, zeros included, from the flat buffer p; a
 * one-call step with STDADK_FLAG_PACK_F32 reads opt->shadow as such a table and its optimiser launch rewrites the
 * copies from the values it has just stepped (the other optimiser entry points always take bf16 tables).  Same
 * products, same summation order: results are bit-identical with and without the copies. */
int stdadk_f32_pack_refresh(const float *p, const stdadk_bf16_shadow *table, stdadk_stream_t stream);

int stdadk_step_advance(int32_t *step_dev, stdadk_stream_t stream);

/* Non-finite guard (ABI 7; scripts/train_st_interp.py:724-733 leaves the epoch at the first batch whose loss is NaN).
 * `loss_watch` is the running objective accumulator the step's kernels add into (the loss_sum of the step-level entry
 * points), `nonfinite_step` a device int32 that starts at 0: the optimiser launch of a step -- which runs after the
 * step's last addition to the accumulator -- stores the 1-based number of the step it applies there when the
 * accumulator is not finite and the word is still 0.  A running sum stays non-finite once it is, so the word ends up
 * holding the FIRST step whose objective was not finite; the host reads it when it reads the loss (no extra sync per
 * step).  Both NULL = off. */
int stdadk_adamw_ema_f32(float *p, const float *g, float *m, float *v, float *ema, int64_t n,
                         float lr, const float *lr_dev, float beta1, float beta2, float eps,
                         float weight_decay, int32_t step, const int32_t *step_dev, float max_norm,
                         const float *sumsq_parts, int32_t n_parts, float grad_mul, float ema_decay,
                         const stdadk_bf16_shadow *shadow, const float *loss_watch, int32_t *nonfinite_step,
                         stdadk_stream_t stream);

/* A9 with two parameter groups in one launch each (learnable knots: the MLP parameters and the knot
 * tensors are clipped on their own norms and stepped with their own learning rates,
 * scripts/train_st_interp.py:470-483,698-705): stdadk_sumsq2_f32 = stdadk_sumsq_f32 on two buffers
 * (step_inc advanced once), stdadk_adamw_ema2_f32 = stdadk_adamw_ema_f32 on two groups. */
typedef struct stdadk_adam_group {
  float *p;                   /* parameters, gradients, Adam moments, EMA shadow (NULL = no EMA) */
  const float *g;
  float *m, *v, *ema;
  int64_t n;
  float lr;                   /* used when lr_dev is NULL                                        */
  const float *lr_dev;
  float max_norm;             /* <= 0: no clipping                                               */
  const float *sumsq_parts;   /* partial sums of squares of g (stdadk_sumsq*_f32)                */
  int32_t n_parts;
  const stdadk_bf16_shadow *shadow;   /* bf16 operand copies to keep current (NULL = none)       */
} stdadk_adam_group;
int stdadk_sumsq2_f32(const float *g0, int64_t n0, float *parts0, const float *g1, int64_t n1,
                      float *parts1, int32_t *step_inc, stdadk_stream_t stream);
int stdadk_adamw_ema2_f32(const stdadk_adam_group *g0, const stdadk_adam_group *g1, float beta1,
                          float beta2, float eps, float weight_decay, int32_t step,
                          const int32_t *step_dev, float grad_mul, float ema_decay,
                          const float *loss_watch, int32_t *nonfinite_step, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Step-level entry points: observations in, predictions / gradients out.
 *
 * One call = the whole of STInterpMLP.forward (st_interp.py:827-882) [+ nn.MSELoss and
 * loss.backward(), scripts/train_st_interp.py:617-621,693].  Two interchangeable paths:
 *   dense  : stdadk_rbf_build_f32 materialises [X|phi|psi] and every layer is a dense MFMA GEMM;
 *   window : for compact-support bases (Wendland, triangular) on the uniform multi-resolution
 *            grid of _init_uniform (st_interp.py:152-185) only the <= 6x6 knots per level that can
 *            be non-zero for an observation are touched: observations are binned into a G x G
 *            cell grid, layer 0 gathers W0^T rows per observation (fused with LayerNorm/ReLU/
 *            Dropout) and every row of dW0^T is accumulated by the one wave that owns it.  phi is
 *            evaluated with the same arithmetic as the dense path; exact zeros are skipped.
 * The window path needs the first layer's weight (and gradient) stored TRANSPOSED, (in,out)
 * row-major (flag STDADK_FLAG_W0_T), hidden[0] in {128, 256} and p <= 16; otherwise, or with
 * STDADK_FLAG_DENSE, the dense path runs (it accepts either W0 layout).
 * ------------------------------------------------------------------------------------------ */
typedef struct stdadk_basis_desc {
  int32_t p;                        /* covariate columns in front of the basis block            */
  int32_t basis;                    /* STDADK_BASIS_*                                            */
  int32_t n_levels;                 /* uniform grid levels; 0 = knots are not a uniform grid     */
  int32_t side[STDADK_MAX_LEVELS];  /* level l is side x side, knot index = ix*side + iy         */
  int64_t Ks, Kt;                   /* spatial / temporal knot counts                            */
  const float *s_centers;           /* [Ks,2]  device                                            */
  const float *s_bw;                /* [Ks]    device                                            */
  const float *t_centers;           /* [Kt]    device                                            */
  const float *t_bw;                /* [Kt]    device                                            */
} stdadk_basis_desc;

#define STDADK_FLAG_DENSE 1 /* force the materialising path                                    */
#define STDADK_FLAG_W0_T 2  /* params->W[0] and grads->W[0] are (in,out) row-major              */
#define STDADK_FLAG_PREBINNED 16 /* window path: the batch was already binned into this workspace by
                              * stdadk_bin_batch_f32 (e.g. on another stream while the previous step
                              * ran); the step entry points skip the binning and ignore coords/t/X/y */
#define STDADK_FLAG_BF16 32 /* BASELINE config C3: the Linear layers AFTER the first run on the bf16 matrix
                              * cores (v_mfma_f32_16x16x32_bf16 in the fused tail kernels, v_mfma_f32_32x32x16_bf16
                              * in the grouped weight-gradient products): operands rounded to bf16 at the
                              * operand boundary (activations as they enter LDS, weights from
                              * params->W_bf16 / WT_bf16), fp32 accumulation, fp32 LayerNorm statistics,
                              * fp32 loss, fp32 master weights / gradients / optimiser state.  phi and psi are
                              * evaluated in fp32 and layer 0 stays fp32 on both paths.  Needs the fused tail
                              * kernels (hidden widths multiples of 16 up to 256); STDADK_E_ARG otherwise */
#define STDADK_FLAG_PACK_F32 128 /* fp32 operands only (with STDADK_FLAG_BF16: STDADK_E_ARG): the fused tail kernels
                              * stream the hidden weights l >= 1 from the fragment-order copies PF / PB that
                              * params->W_bf16[l] / WT_bf16[l] then carry as float * (stdadk_f32_pack_refresh;
                              * every one of them given, 16-byte aligned: STDADK_E_ARG / STDADK_E_ALIGN), and the
                              * one-call step keeps them current through opt->shadow.  Selects no other kernel and
                              * changes no result; needs hidden widths the fused tail kernels take              */
#define STDADK_FLAG_SCATTERED 64 /* the spatial knots are NOT a uniform grid (gmm / random_site initialisers,
                              * st_interp.py:187-343; learnable or fixed): basis->n_levels levels whose SIZES are
                              * basis->side[l] (knot COUNT of level l, any positions; sum = Ks).  The window path
                              * then bins the knots of every level into a 32 x 32 cell grid each step and an
                              * observation gathers the knots of the cells within the level's largest support
                              * radius of its own (same sums as the materialising path, zeros skipped).  Worth it
                              * when the supports are small against the domain; the caller decides (the Python
                              * face: expected candidates <= 35 % of the knots)                                  */
#define STDADK_FLAG_WINDOW 8 /* take the window path whenever it is supported, even for small knot
                              * tables (default: tables under 1024 knots run the materialising
                              * path, which is faster there: a coarse level's few knots each own a
                              * large share of the batch in the per-knot gather of dW0^T)          */
#define STDADK_FLAG_LOG_BW 4 /* learnable knots: basis->s_bw holds LOG-bandwidths (the parameter is
                              * log(bw), used as exp() of it: st_interp.py:101-102,143-148) and the
                              * centres may have moved off the grid.  With n_levels > 0 (the knots
                              * STARTED as the uniform grid, knot k still indexed ix*side+iy) the
                              * window path still applies: every step it widens the candidate
                              * window per level to ceil(max_k (s_k + |c_k - grid_k|_inf)(side-1))
                              * cells, which is guaranteed to contain every knot whose support
                              * reaches an observation; n_levels == 0 runs the materialising path */

/* 1 when the (basis, mlp, flags) combination runs the window path, else 0. */
int32_t stdadk_step_uses_window(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                                int32_t flags);
size_t stdadk_step_workspace_bytes(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                                   int64_t B, int32_t flags);

/* A2-A6 / A10  forward of one batch: y_pred[B,Q] in the caller's row order.
 *   training == 0: eval mode (evaluate_model / dense-grid prediction, scripts/train_st_interp.py:
 *                  884-961,1091-1107,1232-1248,1378-1409): no dropout.
 *   training != 0: train mode; dropout keep-masks come from drop_seed + step_dev[0] (device int32
 *                  step counter, may be NULL; a captured graph draws fresh masks per replay), and
 *                  the workspace keeps what stdadk_backward_f32 needs. */
int stdadk_forward_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                       const stdadk_mlp_tensors *params, const float *coords, const float *t,
                       const float *X, int64_t B, float *y_pred, void *workspace,
                       size_t workspace_bytes, int32_t training, uint64_t drop_seed,
                       const int32_t *step_dev, int32_t flags, stdadk_stream_t stream);

/* A8  loss.backward() (scripts/train_st_interp.py:693) for the batch whose TRAINING forward left
 * its state in `workspace` (same basis/mlp/B/flags/drop_seed/step_dev): dY[B,Q] = dLoss/dy_pred in
 * the caller's row order; every parameter gradient is overwritten in `grads`. */
int stdadk_backward_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                        const stdadk_mlp_tensors *params, const stdadk_mlp_tensors *grads, int64_t B,
                        const float *dY, void *workspace, size_t workspace_bytes, uint64_t drop_seed,
                        const int32_t *step_dev, int32_t flags, stdadk_stream_t stream);

/* N2  learnable knots (DA-STDK; st_interp.py:94-150, scripts/train_st_interp.py:660-672): gradients
 * of the batch loss w.r.t. the spatial centres [Ks,2] and LOG-bandwidths [Ks], for the batch whose
 * backward (stdadk_backward_f32 / stdadk_train_fwd_bwd_f32 with STDADK_FLAG_LOG_BW) has just left dZ
 * of the first layer (materialising path) or the raw per-knot sums (window path: the wave that owns a
 * knot's row of dW0^T accumulates them in the same pass) in `workspace`:
 *   G = dZ0 . W0[:, p:p+Ks]                                  (what autograd sends into phi)
 *   r = |x - c_k| / (exp(log_bw_k) cal);   d_c_k = sum_b G phi'(r) (-(x-c_k)/(|x-c_k| s_k)) (0 at zero
 *   distance, as cdist's backward has it);   d_log_bw_k = sum_b G phi'(r) (-r)
 * The triangular basis at exactly r == 1: the materialising route counts the pair with slope -1, as autograd
 * differentiates clamp(1 - r, min = 0); the window route skips it, because phi == 0 never enters a knot's list.
 * then, when `kt` is given, what the training driver adds on top (all per knot, fixed order):
 *   + penalty_grad_scale * d/dc [ domain_weight  * sum (max(0,-c) + max(0,c-1))^2      (:493-526)
 *                               + movement_weight * sum |c - centers_init|^2 ]         (:528-546)
 *   x exp(-damping_strength * max(|c - centers_init| - damping_threshold, 0))  on d_c  (:111-141, the
 *     gradient hook; applied after the penalties, as the hook sees the accumulated gradient)
 *   loss_sum[0] += penalty_loss_scale * (weighted penalties)            (loss_sum may be NULL)
 * kt == NULL gives the plain data gradient (the module-level autograd path: the hook and the
 * penalties then stay with the caller).  coords are the batch's [B,2] again (unused, may be NULL, on
 * the window path); d_centers / d_log_bw are overwritten. */
typedef struct stdadk_knot_train {
  const float *centers_init;   /* [Ks,2] device; required for damping / movement               */
  int32_t gradient_damping;    /* 0 / 1                                                         */
  float damping_threshold, damping_strength;
  float domain_weight, movement_weight;
  float penalty_grad_scale;    /* 1, or 1/world_size when the ranks' gradients are summed       */
  float penalty_loss_scale;    /* rows*Q of this rank's batch: loss_sum is in those units        */
} stdadk_knot_train;
int stdadk_knot_backward_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                             const stdadk_mlp_tensors *params, const float *coords, int64_t B,
                             void *workspace, size_t workspace_bytes, int32_t flags,
                             const stdadk_knot_train *kt, float *d_centers, float *d_log_bw,
                             float *loss_sum, stdadk_stream_t stream);

/* N2 at module level: the backward of SpatialBasisEmbedding.forward (st_interp.py:433-460) on its own, for callers
 * that differentiate through `model.spatial_basis(coords)` directly rather than through STInterpMLP.forward:
 * d_phi [B, ld] = dLoss/dphi (column k <-> knot k), centres [Ks,2], LOG-bandwidths [Ks] ->
 *   d_centers[k] = sum_b d_phi[b,k] phi'(r) (-(x-c_k)/(|x-c_k| s_k)),  d_log_bw[k] = sum_b d_phi[b,k] phi'(r) (-r)
 * (both overwritten; no damping hook, no penalties: those stay with the caller's autograd). */
size_t stdadk_knot_grad_workspace_bytes(int64_t B, int64_t Ks);
int stdadk_knot_grad_f32(const float *coords, int64_t B, const float *d_phi, int64_t ld,
                         const float *centers, const float *log_bw, int64_t Ks, int32_t basis,
                         float *d_centers, float *d_log_bw, void *workspace, size_t workspace_bytes,
                         stdadk_stream_t stream);

/* A2-A8 in one call: training forward, the batch objective and its gradient, backward:
 *   loss == NULL (nn.MSELoss): loss_sum[0] += sum((y_pred-y)^2), grads = d/dparams of
 *   grad_scale * sum((y_pred-y)^2), y [B,Q];
 *   loss != NULL: the objective of stdadk_loss_f32 (N3), y [B, loss->y_cols].
 * (grad_scale = 1/(rows*Q) of the GLOBAL batch, so summing the ranks' gradients gives the global
 * mean.)  y_pred [B,Q] (caller's row order) is optional: NULL skips writing it.
 * aux_stream (optional, NULL = none): a second stream onto which independent kernels of the step
 * are forked (event fork/join, capturable); on return every kernel has been joined into `stream`. */
int stdadk_train_fwd_bwd_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                             const stdadk_mlp_tensors *params, const stdadk_mlp_tensors *grads,
                             const float *coords, const float *t, const float *X, const float *y,
                             int64_t B, float grad_scale, const stdadk_loss_desc *loss,
                             float *loss_sum, float *y_pred, void *workspace, size_t workspace_bytes,
                             uint64_t drop_seed, const int32_t *step_dev, int32_t flags,
                             stdadk_stream_t stream, stdadk_stream_t aux_stream);

/* A0 + A2-A8: the same step on rows idx[b] (int64, device) of device-RESIDENT observation arrays
 * coords_all [N,2], t_all [N], X_all [N,p], y_all [N, y cols]: the window path's binning reads the
 * rows in place, so the batch producer (scripts/train_st_interp.py:413-460,609-612) costs no launch
 * of its own.  Window path only (STDADK_E_ARG otherwise: gather with stdadk_gather_batch_f32 and call
 * stdadk_train_fwd_bwd_f32).  y_pred, when given, is in batch order (row b <-> idx[b]). */
int stdadk_train_fwd_bwd_indexed_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                                     const stdadk_mlp_tensors *params, const stdadk_mlp_tensors *grads,
                                     const float *coords_all, const float *t_all, const float *X_all,
                                     const float *y_all, const int64_t *idx, int64_t B, float grad_scale,
                                     const stdadk_loss_desc *loss, float *loss_sum, float *y_pred,
                                     void *workspace, size_t workspace_bytes, uint64_t drop_seed,
                                     const int32_t *step_dev, int32_t flags, stdadk_stream_t stream,
                                     stdadk_stream_t aux_stream);

/* Sparsity penalties on the first Linear's weights: STInterpMLP.compute_sparsity_penalty /
 * _compute_penalty_for_block (stnf/models/st_interp.py:724-825) as the batch body adds them to the loss
 * before loss.backward() (scripts/train_st_interp.py:674-691).  A basis function's group is its row of
 * W0^T (w0_t = 1: W0 stored (D, H0), the engine's layout) or its column of W0 (w0_t = 0: (H0, D), the
 * nn.Linear layout); the p covariate rows carry no penalty (:763-765).
 *   ELEMENT       lambda_l1 * sum |w|
 *   GROUP         lambda_group * sum over basis functions of ||w_j||_2
 *   SPARSE_GROUP  both
 * dW0 += grad_scale * d(applied penalties)/dW0 with torch's sub-gradients (sign(0) = 0; an all-zero group has
 * gradient 0); loss_sum += loss_scale * (applied penalties); penalties[0] += spatial, penalties[1] += temporal
 * value (reported whether applied or not, like the reference's dict).  dW0, loss_sum, penalties may be NULL. */
#define STDADK_SPARSITY_NONE 0
#define STDADK_SPARSITY_ELEMENT 1
#define STDADK_SPARSITY_GROUP 2
#define STDADK_SPARSITY_SPARSE_GROUP 3
typedef struct {
  int32_t kind;            /* STDADK_SPARSITY_*                                             */
  float lambda_l1;         /* sparsity_lambda_l1                                            */
  float lambda_group;      /* sparsity_lambda_group                                         */
  int32_t apply_spatial;   /* sparsity_apply_to_spatial  (train_st_interp.py:679,688)       */
  int32_t apply_temporal;  /* sparsity_apply_to_temporal (train_st_interp.py:680,690)       */
} stdadk_sparsity_desc;
int stdadk_sparsity_f32(const stdadk_sparsity_desc *s, const float *W0, float *dW0, int64_t ld,
                        int32_t w0_t, int32_t H0, int32_t p, int32_t Ks, int32_t Kt, float grad_scale,
                        float loss_scale, float *loss_sum, float *penalties, stdadk_stream_t stream);

/* A0 + A2-A9 in ONE call (single GPU): stdadk_train_fwd_bwd(_indexed)_f32, then clip_grad_norm_ +
 * AdamW + EMA (stdadk_sumsq_f32 + stdadk_adamw_ema_f32) on the flat buffers of `opt`, whose gradient
 * buffer [g, g+n) must contain every tensor of `grads` (gaps zero).  Knowing the whole step lets the
 * library take the gradient's squared norm out of the launches that produce it (window path: no
 * separate pass over the gradient); otherwise it runs the separate kernels.  idx may be NULL (rows
 * 0..B-1 of the given arrays).  opt->step_dev (device int32, required) is read by dropout and AdamW and
 * advanced once.  `sparsity` (may be NULL): the first-layer penalties of stdadk_sparsity_f32, their
 * gradient added before clipping and their value x B x Q into loss_sum, like the batch body does.
 * Data-parallel training keeps the split calls: the all-reduce sits between them. */
#define STDADK_GRADSQ_PARTS 512
typedef struct stdadk_optim_desc {
  float *p, *g, *m, *v, *ema;   /* flat fp32 buffers of n elements; ema may be NULL                 */
  int64_t n;
  float lr;                     /* used when lr_dev is NULL                                        */
  const float *lr_dev;
  float beta1, beta2, eps, weight_decay;
  int32_t *step_dev;            /* device step counter (starts at 0)                               */
  float max_norm;               /* clip_grad_norm_ threshold; <= 0: no clipping                    */
  float *sumsq_parts;           /* [STDADK_GRADSQ_PARTS] device scratch                            */
  float ema_decay;
  const stdadk_bf16_shadow *shadow;   /* bf16 operand copies to keep current (NULL = none)           */
  int32_t *nonfinite_step;      /* non-finite guard on the call's loss_sum (see stdadk_adamw_ema_f32), or NULL */
} stdadk_optim_desc;
int stdadk_train_step_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                          const stdadk_mlp_tensors *params, const stdadk_mlp_tensors *grads,
                          const float *coords, const float *t, const float *X, const float *y,
                          const int64_t *idx, int64_t B, float grad_scale, const stdadk_loss_desc *loss,
                          const stdadk_sparsity_desc *sparsity, float *loss_sum, void *workspace,
                          size_t workspace_bytes, uint64_t drop_seed, int32_t flags,
                          const stdadk_optim_desc *opt, stdadk_stream_t stream);

/* stdadk_train_step_f32 on rows `idx` of the RESIDENT arrays, which also prepares the NEXT batch (ABI 8): when the
 * next batch takes the one-launch binning of small batches (window path, next_B <= 8192), rows next_idx of the
 * same arrays are binned into `next_workspace` by extra workgroups of this step's optimiser launch -- no launch of
 * its own, no second stream -- and *next_binned is set to 1: the caller then steps on next_workspace with
 * STDADK_FLAG_PREBINNED (as after stdadk_bin_batch_f32).  Otherwise *next_binned = 0 and nothing was prepared.
 * The resident arrays are always given (also when THIS step runs with STDADK_FLAG_PREBINNED: it reads its rows from
 * `workspace` then); next_y_cols as y_cols of stdadk_bin_batch_f32.  next_workspace must not be `workspace`. */
int stdadk_train_step_next_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                               const stdadk_mlp_tensors *params, const stdadk_mlp_tensors *grads,
                               const float *coords_all, const float *t_all, const float *X_all, const float *y_all,
                               const int64_t *idx, int64_t B, float grad_scale, const stdadk_loss_desc *loss,
                               const stdadk_sparsity_desc *sparsity, float *loss_sum, void *workspace,
                               size_t workspace_bytes, uint64_t drop_seed, int32_t flags, const stdadk_optim_desc *opt,
                               const int64_t *next_idx, int64_t next_B, int32_t next_y_cols, void *next_workspace,
                               size_t next_workspace_bytes, int32_t *next_binned, stdadk_stream_t stream);

/* The one-call step with TWO parameter groups: learnable knots (DA-STDK).  Added under ABI 10 as a new entry point
 * only: no struct, signature or default changes, so STDADK_ABI_VERSION stays 10.
 * = stdadk_train_fwd_bwd(_indexed)_f32 + stdadk_knot_backward_f32 + stdadk_sumsq2_f32 + stdadk_adamw_ema2_f32 of a
 * learnable-knot step, as one call.  The arguments of stdadk_train_step_next_f32, with idx optional (NULL: rows
 * 0..B-1 of the given arrays) and the next batch optional (next_idx, next_B, next_workspace all NULL / 0: none;
 * next_binned may then be NULL), plus
 *   kt                     the knot penalties and the damping hook; NULL = the plain data gradient, as in
 *                          stdadk_knot_backward_f32, whose checks of `kt` apply unchanged
 *   d_centers, d_log_bw    [Ks,2] / [Ks], overwritten.  Both must lie inside [knots->g, knots->g + knots->n);
 *                          elements of that range covered by neither are padding and the caller keeps them zero
 *   knots                  the knot group: p / g / m / v / ema / n, lr / lr_dev and max_norm.  sumsq_parts is a caller
 *                          buffer of STDADK_SUMSQ_PARTS floats (every entry is written), required when max_norm > 0
 *                          and written through although the field is const; n_parts is ignored on input; shadow must be
 *                          NULL
 * `opt` describes the MLP group exactly as for stdadk_train_step_f32 -- [opt->g, opt->g + opt->n) contains every
 * tensor of `grads`, gaps zero, and none of the knot gradients -- and carries what both groups share: betas, eps,
 * weight decay, step_dev, ema_decay and the guard.  The MLP group keeps the guard and, under STDADK_FLAG_BF16,
 * opt->shadow as the table of its bf16 copies.
 * The door needs STDADK_FLAG_LOG_BW, Ks > 0 and at least one hidden layer, and runs on both routes (window,
 * materialising) with every basis and loss that stdadk_train_fwd_bwd_f32 + stdadk_knot_backward_f32 accept.  It refuses
 * STDADK_FLAG_PACK_F32 (STDADK_E_ARG: packed copies are not kept on this path), d_centers / d_log_bw outside the knot
 * group's range, a shadow on the knot group and max_norm > 0 without partials, each with STDADK_E_ARG.  Everything,
 * the next batch included, is validated and planned before the first launch is enqueued: a refused call leaves
 * parameters, moments, EMA, step counter and loss sum untouched.
 * One finishing launch (step_finish_kernel) closes both gradients: its first workgroups run the step's fixed-order
 * sums and leave the squared-norm partials of what they write, where those sums are still pending behind the weight
 * gradients (window route below 49 152 rows); the workgroups behind them finish the knots -- per knot, fixed order,
 * penalty value x penalty_loss_scale into loss_sum -- and each leaves ONE partial, the squares of the d_centers /
 * d_log_bw entries it wrote: at most STDADK_SUMSQ_PARTS knot workgroups stride over the 64-knot tiles, so the knot
 * group's norm is a fixed-order sum of at most 256 partials whatever Ks is.  Where the step's launches do not
 * deliver the MLP group's partials (a sparsity penalty, products outside the grouped launch) its norm is a
 * stdadk_sumsq_f32 over opt->g.  opt->step_dev advances exactly once per call, after the backward and before the
 * optimiser launch (the finishing launch carries the advance).  Then ONE two-group AdamW launch, MLP group first.
 * Next batch: binned by the merged weight-gradient launch when that launch can carry it (window route, the
 * workspaces apart, at most 64 x 64 cells) and *next_binned = 1; in every other case *next_binned = 0 and nothing was
 * prepared (bin it with stdadk_bin_batch_f32).  Under STDADK_DRY_RUN=1 the door validates and plans like every other. */
int stdadk_train_step_knots_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                                const stdadk_mlp_tensors *params, const stdadk_mlp_tensors *grads,
                                const float *coords_all, const float *t_all, const float *X_all, const float *y_all,
                                const int64_t *idx, int64_t B, float grad_scale, const stdadk_loss_desc *loss,
                                const stdadk_sparsity_desc *sparsity, float *loss_sum, void *workspace,
                                size_t workspace_bytes, uint64_t drop_seed, int32_t flags, const stdadk_optim_desc *opt,
                                const int64_t *next_idx, int64_t next_B, int32_t next_y_cols, void *next_workspace,
                                size_t next_workspace_bytes, int32_t *next_binned, const stdadk_knot_train *kt,
                                float *d_centers, float *d_log_bw, const stdadk_adam_group *knots,
                                stdadk_stream_t stream);

/* The one-call step of a model with the delta-reparameterised head (multi-quantile regression with
 * use_delta_reparameterization, the configuration of the reference's Table 4.4), fixed OR learnable knots.  Added
 * under ABI 10 as a new entry point with a struct nobody else uses: no existing struct, signature or default changes,
 * so STDADK_ABI_VERSION stays 10.
 * = stdadk_delta_head_f32 + stdadk_train_fwd_bwd(_indexed)_f32 + stdadk_delta_head_backward_f32 [+
 * stdadk_knot_backward_f32] + clip norm(s) + AdamW/EMA, as one call.  The arguments of stdadk_train_step_knots_f32 plus
 * `head`:
 *   delta, ldd             [Q, ldd] the head's parameter rows (column 0 the bias share, 1..d the weights), inside
 *                          [opt->p, opt->p + opt->n); ldd >= d + 1 with d = the last hidden width, Q = mlp->out_dim >= 2
 *   d_delta, ldg           the same rows of the gradient, overwritten: inside [opt->g, opt->g + opt->n) at the offset
 *                          `delta` has in the parameters, ldg == ldd.  Columns beyond d + 1 are padding, kept zero by
 *                          the caller
 *   lambda_grad, lambda_loss   as stdadk_delta_head_backward_f32 takes them: lambda_grad * dP_nc/d delta is added to
 *                          d_delta, lambda_loss * P_nc(delta) into loss_sum (0: nothing is added)
 * The output layer is DERIVED: params->W[L], b[L] (L = mlp->n_hidden) are rebuilt from `delta` by delta_head_kernel in
 * front of the forward (the first launch of the call's chain behind the validation; only the batch's own
 * preparation may precede it) in every call, so whatever else rewrites the parameters between calls (EMA swaps, a loaded state,
 * evaluation) needs no refresh.  grads->W[L], b[L] are scratch that holds the output layer's gradient after the call, as
 * after stdadk_train_fwd_bwd_f32; they are the one exception to "every tensor of `grads` lies in [opt->g, opt->g + n)":
 * they must lie OUTSIDE it.  The MLP group's clip norm is the norm of the flat gradient: the d_delta entries count, the
 * scratch does not.
 * Knots: kt, d_centers, d_log_bw, knots all NULL = fixed knots, ONE parameter group, and the next batch is carried by
 * stdadk_train_step_next_f32's rules (packed fp32 copies, STDADK_FLAG_PACK_F32, exactly where that door keeps them);
 * all given (kt itself may still be NULL as there) = the two-group step of stdadk_train_step_knots_f32, whose rules apply
 * unchanged, STDADK_FLAG_PACK_F32 refused; d_centers / d_log_bw / knots given only in part is STDADK_E_ARG.
 * A delta step always ends in the finishing launch (step_finish_kernel), which has three kinds of workgroup: the
 * step's fixed-order sums, the knot tiles (none with fixed knots) and ONE head workgroup.  The head workgroup folds
 * (dWo, dbo) into d_delta with the gradient and value of P_nc(delta), in the arithmetic and order of
 * stdadk_delta_head_backward_f32, and leaves ONE clip-norm partial, the squares of what it wrote.  Where a launch in
 * front of the finishing launch runs fixed-order sums anyway (the weight-gradient launch from 49 152 rows, the
 * reductions launch of a learnable step on the materialising route) it finishes the output layer's two sums too and
 * the head workgroup reads them, clearing their slots of squares.  Where the finishing launch itself carries the
 * reductions (window route below 49 152 rows, fixed knots on the materialising route) the head workgroup runs those
 * two sums itself, in the reductions launch's per-element order, before it folds: no workgroup of the launch waits
 * for another.  With fixed knots the launch stands where the reductions launch of the
 * same step without the head stands; where that step has none (window route from 49 152 rows) it is one added launch.
 * opt->step_dev advances exactly once per call, in the finishing launch.
 * Refusals, each STDADK_E_ARG before anything is enqueued (a refused call leaves parameters, moments, EMA, step counter
 * and loss sum untouched): head NULL or Q < 2; ldd < d + 1; delta outside the parameter range or d_delta outside the
 * gradient range or at another offset; ldg != ldd; grads->W[L] / b[L] inside the gradient range; a partial knot
 * description; STDADK_FLAG_PACK_F32 with knots; a shadow on the knot group.  Under STDADK_DRY_RUN=1 the door validates
 * and plans like every other. */
typedef struct stdadk_delta_step {
  const float *delta;
  int64_t ldd;
  float *d_delta;
  int64_t ldg;
  float lambda_grad, lambda_loss;
} stdadk_delta_step;
int stdadk_train_step_delta_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                                const stdadk_mlp_tensors *params, const stdadk_mlp_tensors *grads,
                                const float *coords_all, const float *t_all, const float *X_all, const float *y_all,
                                const int64_t *idx, int64_t B, float grad_scale, const stdadk_loss_desc *loss,
                                const stdadk_sparsity_desc *sparsity, float *loss_sum, void *workspace,
                                size_t workspace_bytes, uint64_t drop_seed, int32_t flags, const stdadk_optim_desc *opt,
                                const int64_t *next_idx, int64_t next_B, int32_t next_y_cols, void *next_workspace,
                                size_t next_workspace_bytes, int32_t *next_binned, const stdadk_knot_train *kt,
                                float *d_centers, float *d_log_bw, const stdadk_adam_group *knots,
                                const stdadk_delta_step *head, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Validation (ABI 9): evaluate_model and the validation half of train_model's epoch
 * (scripts/train_st_interp.py:737-806,884-961) on rows idx[b] (int64, device) of the RESIDENT arrays, forward only.
 *
 * The rows are binned exactly as stdadk_bin_batch_f32 / the indexed training step bin them (window path), or gathered
 * into the workspace (materialising path); the forward runs in eval mode (no dropout, nothing saved for a backward);
 * then a metrics pass reads the predictions and the carried targets in the workspace's own row order and ADDS into
 * `acc`, STDADK_EVAL_SLOTS doubles on the device:
 *   acc[STDADK_EVAL_OBJECTIVE] += batch_weight * sum of the training objective's element terms (NULL loss: squared
 *                                 errors; PINBALL: check loss + prediction-level non-crossing penalty, the arithmetic
 *                                 of stdadk_loss_f32).  batch_weight = 1/(B*Q) makes a sequence of calls accumulate the
 *                                 SUM OF BATCH MEANS the reference divides by len(val_loader), ragged last batch included
 *   acc[STDADK_EVAL_SSE], acc[STDADK_EVAL_SAE] += squared / absolute error of output column `metric_col` against its
 *                                 target (column metric_col of y, or the single column when loss->y_cols == 1)
 *   acc[STDADK_EVAL_ROWS] += B;   acc[STDADK_EVAL_BATCHES] += 1
 *   acc[STDADK_EVAL_CHECK + q] += sum_b max((tau_q-1) e, tau_q e), e = y - y_pred[:,q], q < Q  (tau = 0.5 without a
 *                                 PINBALL descriptor)
 * Deterministic: per-workgroup partial sums in a fixed order, finished in double in a fixed order by one workgroup of
 * a second launch -- the same call on the same data gives the same bits (no atomics).  `params` may point into ANY
 * buffer of the parameters' layout (the live weights or an EMA shadow).  y_pred (optional, NULL = skip): predictions
 * [B,Q] in the caller's order, row b <-> idx[b].  Workspace: stdadk_eval_workspace_bytes (the step workspace -- the full
 * plan of a training step, so that binning and forward are shared as they are -- plus the partials and the gather buffers).  No host read, no allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
#define STDADK_EVAL_OBJECTIVE 0
#define STDADK_EVAL_SSE 1
#define STDADK_EVAL_SAE 2
#define STDADK_EVAL_ROWS 3
#define STDADK_EVAL_BATCHES 4
#define STDADK_EVAL_CHECK 5
#define STDADK_EVAL_SLOTS 16
size_t stdadk_eval_workspace_bytes(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp, int64_t B,
                                   int32_t flags);
int stdadk_eval_indexed_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                            const stdadk_mlp_tensors *params, const float *coords_all, const float *t_all,
                            const float *X_all, const float *y_all, const int64_t *idx, int64_t B,
                            const stdadk_loss_desc *loss, int32_t metric_col, double batch_weight, double *acc,
                            float *y_pred, void *workspace, size_t workspace_bytes, int32_t flags,
                            stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Grid scores (ABI 10): what the reference's driver does last with a trained model -- the (T, S) prediction grid
 * against the full field, split by the train / valid / test masks (scripts/train_st_interp.py:1228-1252
 * `site_mse = nanmean((pred - z)^2, axis=0)`, :1378-1409, :2242, :2551-2560) -- as a reduction on the device, one
 * CHUNK of nT consecutive time slices per call, so that the grid never has to exist as a whole:
 *   y_pred [nT*S][Q]  predictions, time-major: row = ti*S + s (what stdadk_forward_parts_f32 writes)
 *   z      [nT][S]    the field's slice, NaN (or +-inf) = no value: such an entry counts NOWHERE, N included
 *   split  [nT][S]    codes 0..3 (the Python face: 0 none, 1 train, 2 valid, 3 test), NULL = all 0; an entry with
 *                     another code counts nowhere
 * All sums are float64 on the device; every element term is formed in double from operands converted to double:
 *   split_acc [4][STDADK_GRID_SLOTS]  += per split: N; SSE, SAE of column metric_col; CHECK + q, q < Q: the check loss
 *                     max((tau_q-1) e, tau_q e), e = z - y_pred[:,q] (tau = taus_host[q], a HOST array read during the
 *                     call, NULL = 0.5 each); with an interval (lo_col < hi_col; -1/-1 = none) COVER = the count of
 *                     y_pred[lo_col] <= z <= y_pred[hi_col] and WIDTH = the sum of y_pred[hi_col] - y_pred[lo_col]
 *   site_acc  [4][S][3]   (sse, sae, n) += per split and site: a site's slices are added one by one in time order,
 *                     starting from the value already there, so chunked calls give the bits of one call
 *   time_acc  [4][nT][3]  (sse, sae, n) =  per split and time slice of THIS chunk (assigned, not added)
 * Deterministic (no atomics, fixed orders).  Workspace: stdadk_grid_score_workspace_bytes(S, nT) (0 = bad sizes),
 * 8-byte aligned.  S*nT < 2^31.  No host read of device memory, no allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
#define STDADK_GRID_N 0
#define STDADK_GRID_SSE 1
#define STDADK_GRID_SAE 2
#define STDADK_GRID_COVER 3
#define STDADK_GRID_WIDTH 4
#define STDADK_GRID_CHECK 5
#define STDADK_GRID_SLOTS 16
size_t stdadk_grid_score_workspace_bytes(int64_t S, int64_t nT);
int stdadk_grid_score_f32(const float *y_pred, const float *z, const uint8_t *split, int64_t S, int64_t nT,
                          int32_t Q, int32_t metric_col, const float *taus_host, int32_t lo_col, int32_t hi_col,
                          double *split_acc, double *site_acc, double *time_acc, void *workspace,
                          size_t workspace_bytes, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Quantile diagnostics (added under ABI 10: new entry points only, so STDADK_ABI_VERSION stays 10): how good the
 * QUANTILES of a multi-quantile model are on a site x time grid -- reliability of every level, the PIT histogram,
 * how often and how deep the predicted quantiles cross (what the prediction-level penalty, losses.py
 * non_crossing_penalty, and the delta head exist to prevent), CRPS (Eq. 4.6, uniform weights) per site and time --
 * as a reduction on the device beside stdadk_grid_score_f32, with exactly its layout and conventions: one CHUNK of nT
 * consecutive time slices per call,
 *   y_pred [nT*S][Q]  predictions, time-major: row = ti*S + s; finite by contract
 *   z      [nT][S]    the field's slice; a non-finite entry counts NOWHERE
 *   split  [nT][S]    codes 0..3, NULL = all 0; an entry with another code counts nowhere
 *   taus_host [Q]     the levels, a HOST array of float32 read during the call, NULL = 0.5 each
 *   lo_col, hi_col    the interval's columns, lo_col < hi_col, or -1 / -1 for none
 * All sums are float64 on the device.  Every predicate and term is formed in double from operands converted to double,
 * every operation rounded once.  For a counted entry with predictions p_0 .. p_Q-1 and value z:
 *   split_acc [4][STDADK_QD_SLOTS]  += per split:
 *     N               the count of entries
 *     BELOW + q       q < Q: the count of z <= p_q -- the reliability of level q (calibrated: BELOW_q / N ~ tau_q)
 *     PIT + j         j <= Q: the count of entries with #{q : p_q < z} == j -- the histogram over the row's own
 *                     quantile ladder, defined whatever the order of the p_q
 *     CROSS_ROWS      the count of entries with at least one adjacent pair p_q > p_q+1 (strict: equal neighbours do
 *                     not cross)
 *     PAIR + q        q < Q - 1: the count of entries where that adjacent pair crosses
 *     DEPTH1, DEPTH2  the sum over entries and adjacent pairs of max(0, p_q - p_q+1) and of its square; divided by N
 *                     the reference's non_crossing_penalty(y_pred, "mean", power = 1 or 2)
 *     CRPS            the sum over entries of (2 / Q) * (rho_0 + rho_1 + ... + rho_Q-1), added left to right,
 *                     rho_q = max((tau_q - 1) e, tau_q e), e = z - p_q
 *     INSIDE          with an interval, the count of p_lo <= z <= p_hi
 *     (Q == 1: no pairs, the crossing slots stay 0 and PIT has two bins; slots past the used ones are not touched)
 *   site_acc  [4][S][4]   (n, crps, cross_rows, inside) += per split and site, or NULL: a site's slices are added one
 *                     by one in time order, starting from the value already there, so chunked calls give the bits of
 *                     one call (the three counts are integers and are added as such)
 *   time_acc  [4][nT][4]  (n, crps, cross_rows, inside) =  per split and time slice of THIS chunk (assigned), or NULL
 * Deterministic (no atomics, fixed orders).  Workspace: stdadk_quantile_diag_workspace_bytes(S, nT) (0 = bad sizes),
 * 8-byte aligned.  1 <= Q <= STDADK_MAX_Q, S*nT < 2^31.  Errors as stdadk_grid_score_f32: STDADK_E_ARG, _SHAPE,
 * _WORKSPACE, _ALIGN.  No host read of device memory, no allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
#define STDADK_QD_N 0
#define STDADK_QD_BELOW 1
#define STDADK_QD_PIT 9
#define STDADK_QD_CROSS_ROWS 18
#define STDADK_QD_PAIR 19
#define STDADK_QD_DEPTH1 26
#define STDADK_QD_DEPTH2 27
#define STDADK_QD_CRPS 28
#define STDADK_QD_INSIDE 29
#define STDADK_QD_SLOTS 32
size_t stdadk_quantile_diag_workspace_bytes(int64_t S, int64_t nT);
int stdadk_quantile_diag_f32(const float *y_pred, const float *z, const uint8_t *split, int64_t S, int64_t nT,
                             int32_t Q, const float *taus_host, int32_t lo_col, int32_t hi_col,
                             double *split_acc, double *site_acc, double *time_acc,
                             void *workspace, size_t workspace_bytes, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Empirical space-time variograms (added under ABI 10: new entry points only, so STDADK_ABI_VERSION stays 10): has a
 * model captured the spatial and temporal STRUCTURE of the field?  The semivariograms gamma_z(h, u) of the field,
 * gamma_p(h, u) of the prediction (a lower sill than gamma_z's: over-smoothing) and gamma_r(h, u) of the residual
 * (flat: the structure was captured; rising: what is left, and at which range) as one pair reduction on the device
 * over a WHOLE site x time grid, laid out as stdadk_grid_score_f32's:
 *   y_pred [nT*S][ldy]  predictions, time-major: row = ti*S + s; p = y_pred[row][col].  NULL = the field only
 *   z      [nT][S]      the field; split [nT][S] codes 0..3, NULL = all 0
 *   coords [S][2]       the sites
 *   edges2_host [n_bins+1]  a HOST array read during the call: the bin edges as SQUARED distances, strictly
 *                       increasing, edges2[0] >= 0
 * Entries and pairs.  An entry (t, s) is COUNTED when z[t][s] is finite and its split code is 0..3 (the rule of
 * stdadk_grid_score_f32).  For lag u = 0 .. n_lags-1 and t = 0 .. nT-1-u a pair is a = (t, i), b = (t + u, j): at
 * u = 0 the pairs i < j, each unordered pair once and never i = j; at u > 0 every ordered (i, j), i = j included (the
 * purely temporal variogram at distance 0).  A pair counts in split c when both entries are counted and both carry
 * code c; pairs across splits count nowhere.  Lags u >= nT have no pairs.
 * Bins.  d2 = (x_i - x_j)^2 + (y_i - y_j)^2 is formed in float64 from the float32 coordinates, every operation rounded
 * once (two differences, two products, one sum; no fused multiply-add).  The pair falls in bin b when
 * edges2[b] <= d2 < edges2[b+1], otherwise it counts nowhere.  No square root is taken: the bin is decided by exact
 * comparisons, so a host restatement lands every pair in the same bin.
 * Slots.  acc [4][n_lags][n_bins][4] (split, lag, bin, slot), ASSIGNED: one call is one grid (lags reach across
 * slices, so the call is not chunked in time):
 *   N    the count of pairs
 *   SZ   the sum of (z_a - z_b)^2
 *   SP   the sum of (p_a - p_b)^2
 *   SR   the sum of (r_a - r_b)^2, r = z - p formed in double
 * Each difference and each square is formed in double from operands converted to double.  With y_pred NULL, SP and SR
 * are written 0.  The semivariogram of a bin is SUM / (2 N).  The order of summation is the kernel's own but fixed
 * (csrc/variogram.hip: a pair's slices in time order, a tile's pairs of one bin in thread order, a workgroup's tiles in
 * order, the workgroups in order): every sum is of N non-negative terms, so it is within N 2^-52 of the exact sum,
 * relative.  No atomics: the same call gives the same bits.  S = 0 or nT = 0 writes zeros.
 * Errors: n_bins outside 1..64, n_lags outside 1..16, edges2 not strictly increasing or edges2[0] < 0, col outside
 * 0..ldy-1 when y_pred is given, a NULL acc / workspace / edges2_host (or z / coords of a non-empty grid), an output
 * (acc, the workspace) that aliases an input or the other output: STDADK_E_ARG; S*nT >= 2^31: STDADK_E_SHAPE; acc or
 * the workspace not 8-byte aligned: STDADK_E_ALIGN; a workspace below stdadk_variogram_workspace_bytes(S, nT, n_bins,
 * n_lags) (0 = bad sizes): STDADK_E_WORKSPACE.  No host read of device memory, no allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
#define STDADK_VG_N 0
#define STDADK_VG_SZ 1
#define STDADK_VG_SP 2
#define STDADK_VG_SR 3
#define STDADK_VG_MAX_BINS 64
#define STDADK_VG_MAX_LAGS 16
size_t stdadk_variogram_workspace_bytes(int64_t S, int64_t nT, int32_t n_bins, int32_t n_lags);
int stdadk_variogram_f32(const float *y_pred, int64_t ldy, int32_t col, const float *z, const uint8_t *split,
                         const float *coords, int64_t S, int64_t nT, const double *edges2_host, int32_t n_bins,
                         int32_t n_lags, double *acc, void *workspace, size_t workspace_bytes,
                         stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Basis diagnostics (added under ABI 10: new entry points only, so STDADK_ABI_VERSION stays 10): what did the BASIS
 * do?  How much training data sits in each knot's support, which sites does no knot of a level cover, which basis
 * functions did group lasso switch off.  stdadk_basis_diag_f32 is one sites x knots pair reduction on the device over
 * the LIVE knot tables; stdadk_group_norms_f32 gives the first Linear's group norms the sparsity analysis starts from.
 *   s_centers [Ks][2], s_bw [Ks]   float32, device: the tables as stdadk_basis_desc carries them (bandwidths, not
 *                       their logarithms)
 *   basis               STDADK_BASIS_*
 *   level_sizes_host [n_levels]  a HOST array read during the call: the knot count of every level, each >= 0, summing
 *                       to Ks; 1..STDADK_MAX_LEVELS levels.  Level l holds the knots after those of levels < l: grid
 *                       and scattered tables alike
 *   coords [S][2]       float32, device: the sites
 *   w [S]               float64 or NULL (= all 1): the site's weight, e.g. its number of training observations
 *   v [S]               float64 or NULL: a site value, e.g. its test MSE
 *   rho                 the support radius in units of the scaled radius r, finite and > 0
 * Pairs.  For site i and knot k, d2 = (x_i - cx_k)^2 + (y_i - cy_k)^2 is formed in float64 from the float32 operands,
 * every operation rounded once (two differences, two products, one sum; no fused multiply-add).  With cal the double
 * literal 1.0 (Wendland) / 0.223477 (Gaussian) / 0.654714 (triangular): den_k = (double)bw_k * cal,
 * s_k = den_k * rho, R2_k = s_k * s_k, each rounded once.  The pair is IN SUPPORT iff d2 < R2_k: an exact comparison,
 * so a host restatement makes the same decision for every pair (a NaN d2 is in no support and is no minimum).  For a
 * pair in support r = sqrt(d2) / den_k and phi(r) is formed in double with the formulas of csrc/basis.h:
 *   Wendland    r' = min(r, 1), om = 1 - r', om2 = om om, phi = (om2 om2 om2) ((35 r' + 18) r' + 3) / 3
 *   Gaussian    exp(-0.5 r r)
 *   triangular  max(1 - r, 0)
 * Pairs out of support contribute nothing: for the Gaussian kind the tail beyond rho is dropped by contract.
 * Outputs, float64, both ASSIGNED:
 *   knot_acc [Ks][7], over the sites whose w_i is finite and > 0 (all of them without w):
 *     N      the count of such sites in support
 *     W      the sum of w
 *     SPHI   the sum of w phi
 *     SPHI2  the sum of (w phi) phi
 *     SV     the sum of (w phi) v over the sites in support with a finite v
 *     WV     the sum of w phi over the same sites: the phi-weighted mean of v around the knot is SV / WV
 *     NEAR2  the minimum d2 to any such site, in support or not; +inf when there is none
 *     Without v, SV = WV = 0.
 *   site_acc [S][n_levels][3], for EVERY site whatever its weight, per level:
 *     COVER  the count of the level's knots whose support holds the site
 *     SPHI   the sum of phi over them
 *     NEAR2  the minimum d2 to a knot of the level; +inf for a level without knots
 * The order of summation is the kernel's own but fixed by the sizes alone (csrc/basis_diag.hip: of a knot's sites in a
 * span each of four waves adds every fourth sub-chunk of 64 in site order, then the waves in order, then the spans in
 * order; of a site's knots of a level each wave adds its quarter of every chunk of 256 in knot order, then the waves
 * in order): every sum is of n non-negative terms (v aside), so it is within n 2^-52 of the exact sum, relative.  No atomics: the same call gives the
 * same bits.  Ks = 0 writes the sites' neutral rows (0, 0, +inf), S = 0 the knots' (zeros, NEAR2 = +inf).
 * Errors: S or Ks outside 0..2^31-1, an unknown basis, n_levels outside 1..STDADK_MAX_LEVELS, level sizes that are
 * negative or do not sum to Ks, rho not finite or <= 0, a NULL level_sizes_host / workspace (or s_centers / s_bw /
 * knot_acc with Ks > 0, coords / site_acc with S > 0), an output (knot_acc, site_acc, the workspace) that aliases an
 * input or another output: STDADK_E_ARG; knot_acc, site_acc, w, v or the workspace not 8-byte aligned: STDADK_E_ALIGN; a
 * workspace below stdadk_basis_diag_workspace_bytes(S, Ks) (0 = bad sizes): STDADK_E_WORKSPACE.  No host read of device
 * memory, no allocation, capturable.
 *
 * stdadk_group_norms_f32: for the basis functions col0 .. col0 + n - 1 of the first Linear the float64 sum of squares
 * of the function's group of H weights, ASSIGNED to out [n] (the norm is its square root; the spatial and the temporal
 * block are adjacent columns after the p covariates, so one call covers both).  transposed = 0: W0 is (H, D) row-major
 * with row stride ld >= col0 + n and the group is a COLUMN; transposed = 1 (the meaning of STDADK_FLAG_W0_T): W0 is
 * (D, H) row-major with row stride ld >= H and the group is a ROW.  Each weight is converted to double and squared
 * there; the order is fixed (a column's rows in order; a row's terms h, h + 64, ... per lane in order, the 64 lanes
 * by a fixed tree).  n = 0 does nothing.  Errors: H < 1, col0 < 0, n < 0, col0 + n >= 2^31, transposed not 0 / 1, an
 * ld shorter than a row, a NULL pointer, out inside W0: STDADK_E_ARG; out not 8-byte aligned: STDADK_E_ALIGN.
 * ------------------------------------------------------------------------------------------ */
#define STDADK_BD_KNOT_SLOTS 7
#define STDADK_BD_K_N 0
#define STDADK_BD_K_W 1
#define STDADK_BD_K_SPHI 2
#define STDADK_BD_K_SPHI2 3
#define STDADK_BD_K_SV 4
#define STDADK_BD_K_WV 5
#define STDADK_BD_K_NEAR2 6
#define STDADK_BD_SITE_SLOTS 3
#define STDADK_BD_S_COVER 0
#define STDADK_BD_S_SPHI 1
#define STDADK_BD_S_NEAR2 2
size_t stdadk_basis_diag_workspace_bytes(int64_t S, int64_t Ks);
int stdadk_basis_diag_f32(const float *s_centers, const float *s_bw, int64_t Ks, int32_t basis,
                          const int64_t *level_sizes_host, int32_t n_levels, const float *coords, int64_t S,
                          const double *w, const double *v, double rho, double *knot_acc, double *site_acc,
                          void *workspace, size_t workspace_bytes, stdadk_stream_t stream);
int stdadk_group_norms_f32(const float *W0, int64_t ld, int32_t transposed, int32_t H, int64_t col0, int64_t n,
                           double *out, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Split-conformal calibration (added under ABI 10: new entry points only, so STDADK_ABI_VERSION stays 10): the
 * conformity scores of a site x time grid as an ordered compaction, and exact order statistics of them without a sort.
 * Shifting a model's quantiles by one order statistic of the calibration split's scores gives finite-sample marginal
 * coverage whatever the model learned (conformalized quantile regression; the Python face is stnf.calibration).
 *
 * stdadk_conformal_scores_f32: one CHUNK of nT consecutive time slices, laid out as stdadk_grid_score_f32's:
 *   y_pred [nT*S][Q]  predictions, time-major: row = ti*S + s; finite by contract
 *   z      [nT][S]    the field's slice; a non-finite entry is no member of any segment
 *   split  [nT][S]    codes 0..255, NULL = all 0 (a validation set is then passed as nT = 1, S = N)
 *   cols_host [C][3]  a HOST array of int32 read during the call, 1 <= C <= STDADK_CONFORMAL_MAX_COLS: per score column
 *                     (kind, col_a, col_b), col_b read for CQR only.  With p = the row's predictions, every operation
 *                     in float32 and rounded once (the bits of numpy float32 arithmetic):
 *                       STDADK_CONFORMAL_RESID   z - p[col_a]
 *                       STDADK_CONFORMAL_CQR     max(p[col_a] - z, z - p[col_b])
 *                       STDADK_CONFORMAL_ABS     |z - p[col_a]|
 *   codes_host [G]    a HOST array of int32, 1 <= G <= STDADK_CONFORMAL_MAX_SEGMENTS: the split code of every segment
 *   scores [G][C][cap]  float32: segment g, column c holds its scores from index 0 on
 *   count  [G]        int64, device: the members segment g holds already.  READ as the first append position (a negative
 *                     value as 0) and ADVANCED by the chunk's members at the end of the call, saturating at cap
 *   overflow [G]      int32, device: SET to 1 when the chunk's members did not all fit; otherwise not touched
 * An entry is a MEMBER of segment g when z is finite and split == codes_host[g].  Members are appended in time-major,
 * then site order -- numpy's scores[mask] order -- so chunked calls over a grid leave the bytes of one call.  A member
 * whose position is >= cap is dropped: nothing is ever written outside a segment, and what was written is the correct
 * prefix.  Positions come from per-run member counts (a run is 1024 consecutive rows), an exclusive scan over the
 * chunk's runs and ballot ranks inside a run: no atomics, the same call gives the same bytes.
 * Workspace: stdadk_conformal_scores_workspace_bytes(S, nT) (0 = bad sizes), 8-byte aligned.  S = 0 or nT = 0 does
 * nothing.  Errors: a negative size or capacity, Q outside 1..STDADK_MAX_Q, C or G outside their range, an unknown kind,
 * a prediction column outside 0..Q-1, a code outside 0..255, a NULL pointer: STDADK_E_ARG; S*nT or cap >= 2^31:
 * STDADK_E_SHAPE; count not 8-byte, scores or overflow not 4-byte aligned, the workspace not 8-byte aligned:
 * STDADK_E_ALIGN; a workspace too small: STDADK_E_WORKSPACE.  No host read of device memory, no allocation, capturable.
 *
 * stdadk_select_f32: exact order statistics of columns of finite float32 values.
 *   keys              device: column c is keys[c*stride .. c*stride + n - 1], 1 <= C <= STDADK_CONFORMAL_MAX_COLS
 *   n_dev             int64, device: n, the SAME for every column (e.g. count[g] of the scores call: no host read in
 *                     between).  n_max: the host's bound on it, n_max <= stride, n_max < 2^31; a device value outside
 *                     0..n_max is read as the nearer end
 *   sel_col_host, sel_rank_host, sel_beta_host [n_sel]  HOST arrays, 1 <= n_sel <= STDADK_SELECT_MAX: the column; the
 *                     0-based rank, or a negative rank and a level beta in [0, 1] (sel_beta_host may be NULL when every
 *                     rank is given).  With a level the 1-based rank is k = ceil((n + 1) * beta), that one product
 *                     and the ceiling evaluated in IEEE double, k below 1 taken as 1; the 0-based rank is k - 1
 *   value [n_sel]     float32: the rank-th smallest value of the column (0-based; equal values count as often as they
 *                     occur; -0 is returned as +0)
 *   rank_used [n_sel] int64: the 0-based rank that was used
 * A rank >= n (k > n, n = 0) gives value = +inf and rank_used = -1: conformal's "not enough calibration data".
 * Method: radix select.  A value's key is its bits with -0 canonicalised to +0, all bits flipped for negatives and the
 * sign bit flipped otherwise: unsigned order = float order.  Four passes of 8 bits, most significant first.  A pass
 * reads the data once for ALL selections of all columns: per workgroup one set of histograms (16 x 256 x uint32) in LDS,
 * integer LDS atomics on the keys whose higher digits match the selection's prefix, integer global atomics to merge
 * the workgroups; then one wave per selection picks the bin where the cumulative count crosses the remaining rank and
 * clears the histogram.  After the last pass the prefix is the key of the value; the data is never searched for it.
 * Integer counts do not depend on the order of arrival: the same call gives the same bits.
 * Workspace: stdadk_select_workspace_bytes(n_sel) (0 = n_sel out of range), 8-byte aligned.  Errors: n_sel or C out of
 * range, a column outside 0..C-1, a negative rank without a level in [0, 1], a negative n_max or stride, a NULL
 * pointer: STDADK_E_ARG; n_max >= 2^31 or stride < n_max: STDADK_E_SHAPE; n_dev or rank_used not 8-byte, keys or value not
 * 4-byte aligned, the workspace not 8-byte aligned: STDADK_E_ALIGN; a workspace too small: STDADK_E_WORKSPACE.  No host
 * read of device memory, no allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
#define STDADK_CONFORMAL_RESID 0
#define STDADK_CONFORMAL_CQR 1
#define STDADK_CONFORMAL_ABS 2
#define STDADK_CONFORMAL_MAX_COLS 8
#define STDADK_CONFORMAL_MAX_SEGMENTS 2
#define STDADK_SELECT_MAX 16
size_t stdadk_conformal_scores_workspace_bytes(int64_t S, int64_t nT);
int stdadk_conformal_scores_f32(const float *y_pred, const float *z, const uint8_t *split, int64_t S, int64_t nT,
                                int32_t Q, const int32_t *cols_host, int32_t C, const int32_t *codes_host, int32_t G,
                                float *scores, int64_t cap, int64_t *count, int32_t *overflow, void *workspace,
                                size_t workspace_bytes, stdadk_stream_t stream);
size_t stdadk_select_workspace_bytes(int32_t n_sel);
int stdadk_select_f32(const float *keys, int64_t stride, int32_t C, const int64_t *n_dev, int64_t n_max,
                      const int32_t *sel_col_host, const int64_t *sel_rank_host, const double *sel_beta_host,
                      int32_t n_sel, float *value, int64_t *rank_used, void *workspace, size_t workspace_bytes,
                      stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Neighbour tables (added under ABI 10: new entry points only, so STDADK_ABI_VERSION stays 10): the k nearest of a set
 * of sites, exactly, and a table applied to a field -- the baselines "copy the nearest observed site" and
 * inverse-distance weighting (IDW) a model's scores stand next to (stnf.utils.baselines), and the nearest-site raster
 * of a per-site map.
 *
 * stdadk_knn_f32: the search, brute force.
 *   q [M][2]            float32, device: the targets
 *   coords [S][2]       float32, device: the candidate sources
 *   src [nM][S]         uint8, device, or NULL (= every site; nM must then be 1): slice m's sources are the sites with
 *                       src != 0
 *   k                   1 .. STDADK_KNN_MAX_K
 *   exclude_self        0 / 1; 1 requires M == S and skips source j for target j (leave-one-site-out)
 *   nbr_idx [nM][M][k]  int32, ASSIGNED
 *   nbr_d2  [nM][M][k]  float64, ASSIGNED
 * For target j and source i, d2 = (qx - cx)^2 + (qy - cy)^2 is formed in float64 from the float32 operands, every
 * operation rounded once (two differences, two products, one sum; no fused multiply-add).  A NaN d2 is never a
 * neighbour; a d2 of +inf is one like any other.  The neighbours of (m, j) are the k smallest sources of slice m in the
 * TOTAL order (d2, source index) -- equal distances go to the lower index -- written in that order; a host
 * restatement is np.lexsort((index, d2))[:k].  When fewer than k sources exist the tail is idx = -1, d2 = +inf.
 * Because the order is total the answer does not depend on how the kernel partitions the sources (csrc/knn.hip: over
 * four waves, and over source spans when targets x slices alone would leave the device idle): the same call gives the
 * same bits, and so does any other launch plan.  M = 0 or nM = 0 writes nothing; S = 0 writes the neutral rows.
 * Errors: M, S or nM outside 0..2^31-1, k outside 1..STDADK_KNN_MAX_K, exclude_self not 0 / 1 or set with M != S,
 * src == NULL with nM != 1 (unless nM*S == 0: no flag to read), a NULL q / nbr_idx / nbr_d2 (with M, nM > 0), coords (with S > 0) or workspace, an output
 * (nbr_idx, nbr_d2, the workspace) that aliases an input or another output: STDADK_E_ARG; nM*M*k >= 2^31:
 * STDADK_E_SHAPE; nbr_d2 or the workspace not 8-byte, nbr_idx, q or coords not 4-byte aligned: STDADK_E_ALIGN; a
 * workspace below stdadk_knn_workspace_bytes(M, S, nM, k) (0 = bad sizes): STDADK_E_WORKSPACE.  No host read of device
 * memory, no allocation, capturable.
 *
 * stdadk_knn_apply_f32: a table applied to a field.
 *   nbr_idx, nbr_d2 [nM][M][k_tab]   a table of the search; nM == 1 (one table for every slice) or nM == nT
 *   k                   1 .. k_tab: the first k entries of a row are used (a prefix of the order is the order)
 *   z [nT][S]           float32: the field's slices
 *   power               0, 1, 2, 3 or 4
 *   nearest [nT][M], idw [nT][M]     float32, ASSIGNED; either may be NULL (not both)
 * For entry (ti, j) the row is that of slice m = (nM == 1 ? 0 : ti).  An entry of the row counts when 0 <= idx < S
 * (the search's tail of -1 does not; an index >= S is never dereferenced).  No entry counts: NaN in both outputs.
 *   nearest  z[ti][idx] of the first entry that counts, the bits copied.
 *   idw      if the first entry that counts has d2 == 0: the mean of z over the leading run of entries with d2 == 0 --
 *            the sum in double in row order, ONE division, rounded to float32 once.  Otherwise, over the entries that
 *            count in row order, w = 1 (power 0), 1/sqrt(d2) (1), 1/d2 (2), 1/(d2 sqrt(d2)) (3), 1/(d2 d2) (4), every
 *            operation an IEEE double operation rounded once (division and square root correctly rounded); then
 *            num += w z and den += w sequentially (the product rounded, then the sum), and idw = (float)(num / den).
 * numpy float64 restates every output bit for bit.  A non-finite z at a used neighbour propagates: callers exclude such
 * entries through src.
 * Errors: M, S, nT, nM or k_tab outside 0..2^31-1, nM not 1 and not nT, k outside 1..k_tab or k_tab above
 * STDADK_KNN_MAX_K, power outside 0..4, a NULL table or z, or nearest and idw both NULL (with nT, M > 0), an output that
 * aliases an input or the other output: STDADK_E_ARG; nT*M, nT*S or nM*M*k_tab >= 2^31: STDADK_E_SHAPE; nbr_d2 not
 * 8-byte, nbr_idx, z, nearest or idw not 4-byte aligned: STDADK_E_ALIGN.  nT = 0 or M = 0 writes nothing.  No
 * workspace, no host read of device memory, no allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
#define STDADK_KNN_MAX_K 16
size_t stdadk_knn_workspace_bytes(int64_t M, int64_t S, int64_t nM, int32_t k);
int stdadk_knn_f32(const float *q, int64_t M, const float *coords, int64_t S, const uint8_t *src, int64_t nM, int32_t k,
                   int32_t exclude_self, int32_t *nbr_idx, double *nbr_d2, void *workspace, size_t workspace_bytes,
                   stdadk_stream_t stream);
int stdadk_knn_apply_f32(const int32_t *nbr_idx, const double *nbr_d2, int64_t nM, int64_t M, int32_t k_tab, int32_t k,
                         const float *z, int64_t nT, int64_t S, int32_t power, float *nearest, float *idw,
                         stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same table by a cell-binned search (added under ABI 10: new entry points only, so STDADK_ABI_VERSION stays 10).
 *
 * stdadk_knn_cells_f32 takes exactly the parameter list of stdadk_knn_f32 and, for every input that entry accepts,
 * ASSIGNS the same nbr_idx and nbr_d2, bit for bit: NaN and inf coordinates, short rows (-1 / +inf), S = 0 and slices
 * without sources, exclude_self, and the rows in the caller's target order included.  It refuses the same inputs with
 * the same codes; its workspace is stdadk_knn_cells_workspace_bytes(M, S, nM, k) (0 = bad sizes; below it:
 * STDADK_E_WORKSPACE).  No host read of device memory, no allocation, capturable: the plan follows from M, S, nM and k
 * or is computed on the device.
 * The plan (csrc/knn_cells.hip): the sites are binned once into a uniform grid over the box of their finite coordinates,
 * the side chosen from S alone; the targets are sorted by cell; a wave of 64 cell-adjacent targets walks the cells of
 * its rectangle and then one frame of cells per ring.  A source is skipped only when a lower bound of its d2, formed by
 * the same rounded operations from the exact extreme coordinate not yet met, is STRICTLY above the target's current
 * k-th distance; an equal bound visits, and a NaN or inf target visits everything.  The order inside a cell may differ
 * from run to run; the table cannot, because the order (d2, source index) is total.  What it costs is decided by the
 * data: sites spread evenly over their box are its case; a slice that uses few of the sites, or sites in a few tight
 * clusters, walks many rings (or crowded cells) and can be slower than the brute-force call.
 * ------------------------------------------------------------------------------------------ */
size_t stdadk_knn_cells_workspace_bytes(int64_t M, int64_t S, int64_t nM, int32_t k);
int stdadk_knn_cells_f32(const float *q, int64_t M, const float *coords, int64_t S, const uint8_t *src, int64_t nM,
                         int32_t k, int32_t exclude_self, int32_t *nbr_idx, double *nbr_d2, void *workspace,
                         size_t workspace_bytes, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Local ordinary kriging on a neighbour table (added under ABI 10: new entry points only, so STDADK_ABI_VERSION stays
 * 10): the baseline a geostatistics user asks for first (stnf.utils.kriging, stnf.utils.baselines), with a variance, so
 * that Gaussian quantiles of it go through stdadk_grid_score_f32 and stdadk_quantile_diag_f32 unchanged.  One
 * variogram model for the whole table (no anisotropy, no drift, no covariates, no global solve).
 *
 * stdadk_krige_weights_f64: per row of a table the ordinary-kriging weights and variance.
 *   nbr_idx, nbr_d2 [nM][M][k_tab]   a table of stdadk_knn_f32 (device); the first k entries of a row are used
 *   coords [S][2]       float32, device: the sites the indices name
 *   model               STDADK_KRIGE_EXPONENTIAL rho = exp(-r), _SPHERICAL rho = 1 - r (1.5 - 0.5 r r) for d < range
 *                       and 0 for d >= range, _GAUSSIAN rho = exp(-(r r)); d = sqrt(d2) and r = d / range correctly
 *                       rounded, every further operation rounded once in the order written (t = 0.5 (r r), 1.5 - t,
 *                       r (..), 1 - (..)); exp is the device library's (the host's differs in its last bits)
 *   nugget, psill, range   the model: gamma(h) = nugget + psill (1 - rho(h)), i.e. covariance psill rho(h)
 *   w [nM][M][k], var [nM][M]   float64, ASSIGNED
 * ENTRIES.  Of row (m, j) the entries that COUNT are those of the first k with 0 <= idx < S (stdadk_knn_apply_f32's
 * rule), taken in row order.  Two entries are COINCIDENT when the d2 between their sources, formed from `coords` as the
 * search forms it (two differences, two products, one sum, each rounded once), is exactly 0.  Coincident entries form a
 * group, represented by its first member; `members` is its size.  The unknowns of the row's system are the groups.
 * SYSTEM.  K_ab = psill rho(d_ab) + [a == b] nugget / members_a (the diagonal is psill + nugget / members, one
 * division, one sum; rho(0) = 1 is not evaluated), k_a = psill rho(d_a0) with d_a0 from nbr_d2.  The nugget is on the
 * diagonal only: a target that coincides with a source does NOT reproduce it when nugget > 0 -- the prediction is of
 * the smooth signal.
 * SOLVE.  Cholesky K = L L^T in a FIXED order: every element is K_ab minus the products L_ac L_bc in increasing c, each
 * product rounded, then each subtraction (no fused multiply-add), then one division by L_bb, or one square root on the
 * diagonal.  L y = r for r = 1 and r = k the same way (r_a minus L_ac y_c in increasing c, one division); L^T x = y
 * from the last unknown down, x_a = (y_a minus L_ca x_c in DECREASING c) / L_aa.  u = K^-1 1, v = K^-1 k.
 * WEIGHTS.  mu = (sum v - 1) / sum u (sums in row order from 0), w = v - mu u, var = ((nugget + psill) - sum w_a k_a)
 * - mu with the sum in row order: the variance of a new noisy observation, not clamped.  A group's weight is written
 * to each of its members as w / members (one division); entries that do not count get w = 0.
 * DEGENERATE ROWS.  No entry counts: w = 0, var = NaN.  A pivot (the value under the square root) that is <= 0 or not
 * finite: every w of the row and var are NaN -- the row is singular and the call says so.
 * Deterministic: no atomics, fixed orders; the same call gives the same bits.  With the spherical model numpy float64
 * restates every bit (stnf.utils.kriging.kriging_weights_host).
 * Errors: M, S or nM outside 0..2^31-1, model outside 0..2, nugget < 0, psill < 0, nugget + psill == 0, range <= 0 or
 * any of them not finite, k outside 1..k_tab or k_tab outside 1..STDADK_KNN_MAX_K, a NULL pointer (with nM, M > 0;
 * coords with S > 0), an output that aliases an input or the other output: STDADK_E_ARG; nM*M*k_tab >= 2^31:
 * STDADK_E_SHAPE; nbr_d2, w or var not 8-byte, nbr_idx or coords not 4-byte aligned: STDADK_E_ALIGN.  M = 0 or nM = 0
 * writes nothing.  No workspace, no host read of device memory, no allocation, capturable.
 *
 * stdadk_krige_apply_f32: the weights applied to a field, with Gaussian quantiles.
 *   nbr_idx [nM][M][k_tab], w [nM][M][k], var [nM][M]   nM == 1 (one table for every slice) or nM == nT
 *   z [nT][S]           float32: the field's slices
 *   zq_host [Q]         float64 on the HOST, read during the call: the standard-normal quantile of every wanted
 *                       level, 0 for the mean; 1 <= Q <= STDADK_KRIGE_MAX_COLS
 *   out [nT*M][ldo]     float32, columns 0 .. Q-1 ASSIGNED, ldo >= Q: the y_pred layout of stdadk_grid_score_f32
 * For entry (ti, j): p = sum_a w_a (double)z[ti][idx_a] over the entries that count in row order from 0 (each product
 * rounded, then the sum), sd = sqrt(max(var, 0)), out[(ti M + j) ldo + c] = (float)(p + zq[c] sd) (the product
 * rounded, then the sum, then the conversion).  A row with var NaN gives NaN in every column.  numpy float64 restates
 * every bit, given w and var (stnf.utils.kriging.kriging_apply_host).
 * Errors: M, S, nT or nM outside 0..2^31-1, nM not 1 and not nT, k or k_tab as above, Q outside 1..8, ldo < Q or
 * >= 2^31, a NULL or non-finite zq_host, a NULL pointer (with nT, M > 0; z with S > 0), out aliasing an input:
 * STDADK_E_ARG; nT*M, nT*S or nM*M*k_tab >= 2^31: STDADK_E_SHAPE; w or var not 8-byte, nbr_idx, z or out not 4-byte
 * aligned: STDADK_E_ALIGN.  nT = 0 or M = 0 writes nothing.  No workspace, no host read of device memory, no
 * allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
#define STDADK_KRIGE_EXPONENTIAL 0
#define STDADK_KRIGE_SPHERICAL 1
#define STDADK_KRIGE_GAUSSIAN 2
#define STDADK_KRIGE_MAX_COLS 8
int stdadk_krige_weights_f64(const int32_t *nbr_idx, const double *nbr_d2, int64_t nM, int64_t M, int32_t k_tab,
                             int32_t k, const float *coords, int64_t S, int32_t model, double nugget, double psill,
                             double range, double *w, double *var, stdadk_stream_t stream);
int stdadk_krige_apply_f32(const int32_t *nbr_idx, const double *w, const double *var, int64_t nM, int64_t M,
                           int32_t k_tab, int32_t k, const float *z, int64_t nT, int64_t S, const double *zq_host,
                           int32_t Q, float *out, int64_t ldo, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Knot initialiser (added under ABI 10: new entry points only, nothing existing changes, so STDADK_ABI_VERSION stays
 * 10): ONE EM iteration of the spherical Gaussian mixture in two dimensions behind `spatial_init_method: gmm`
 * (stnf/models/st_interp.py:187-266 fits sklearn.mixture.GaussianMixture(covariance_type='spherical') on the host),
 * entirely in float64.  All pointers are device pointers:
 *   X [n][2] samples; w [k], mu [k][2], var [k] the current parameters; *_out the next ones; lower_bound [1].
 * E-step on the parameters given (d = 2, the direct squared distance):
 *   lp_ij = log w_j - 0.5 (d log 2pi + |x_i - mu_j|^2 / var_j) - 0.5 d log var_j,   lpn_i = logsumexp_j lp_ij,
 *   lower_bound = (1/n) sum_i lpn_i
 * M-step with r_ij = exp(lp_ij - lpn_i), eps = 2^-52:
 *   nk_j = sum_i r_ij + 10 eps,  mu_out_j = sum_i r_ij x_i / nk_j,
 *   var_out_j = sum_i r_ij |x_i - mu_out_j|^2 / (d nk_j) + reg_covar   (about the NEW mean, non-negative terms),
 *   w_out_j = nk_j / sum_j nk_j
 * A component no sample reaches (every r_ij == 0) gives mu_out_j = 0, var_out_j = reg_covar and a finite w_out_j.
 * The responsibilities are never stored (each pass recomputes lp_ij; lpn lives in the workspace).  Outputs must not
 * alias inputs, each other or the workspace (STDADK_E_ARG): the caller ping-pongs two parameter sets.
 * 1 <= n < 2^31, 1 <= k <= 65536, reg_covar > 0.  Deterministic (no atomics, fixed orders).  Workspace:
 * stdadk_gmm_workspace_bytes(n, k) (0 = bad sizes), 8-byte aligned.  No host read of device memory, no allocation,
 * capturable.
 * ------------------------------------------------------------------------------------------ */
size_t stdadk_gmm_workspace_bytes(int64_t n, int32_t k);
int stdadk_gmm_em_f64(const double *X, int64_t n, int32_t k, const double *w, const double *mu, const double *var,
                      double reg_covar, double *w_out, double *mu_out, double *var_out, double *lower_bound,
                      void *workspace, size_t workspace_bytes, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Knot initialiser `spatial_init_method: kmeans_balanced` (added under ABI 10: new entry points only, so
 * STDADK_ABI_VERSION stays 10): ONE iteration of size-constrained k-means in two dimensions.  The reference
 * (stnf/models/st_interp.py:345-431) fits the k_means_constrained package's KMeansConstrained; this library states a
 * contract of its own and does NOT claim that package's bits: the knots are a size-constrained k-means fit under
 * the contract below, nothing more.
 *
 * The fit (host side, stnf.knot_init.fit_balanced_kmeans), all float64:
 *   points   P = at most 10 000 rows of the training coordinates (the reference's global-numpy-RNG draw, :367-375)
 *   bounds   of a level of k knots on n = len(P) points: lo = max(1, n / k - 1), hi = n / k + n % k (integer division;
 *            :379-385); k > n is an error, and k lo <= n <= k hi always holds otherwise
 *   restarts the three seed index arrays of sklearn's kmeans_plusplus on one RandomState(42), in sequence; the centres
 *            start at the seed rows
 *   one restart, at most 100 iterations:  tol = 1e-4 mean(var(P, axis 0)), mu = P[seeds], then
 *            E: labels = the assignment minimising sum_i |x_i - mu_labels[i]|^2 subject to lo <= |cluster j| <= hi for
 *               every j -- the EXACT optimum; inertia = that minimum
 *            M: mu_new[j] = mean of the members of j (none is empty: lo >= 1), a fixed summation order
 *            shift = sum |mu_new - mu|^2; mu = mu_new; stop when shift <= tol
 *            the result is mu and the inertia of the last E-step
 *   the restart with the lowest inertia is kept, the first on a tie
 *   knots    centres = mu as float32; bandwidth = 2.5 x the mean distance to the min(4, k - 1) nearest other centres of
 *            the level, the grid bandwidth of n_centers[0] for k == 1 (:400-422, the arithmetic of random_site)
 *
 * This call is one iteration: E on mu, M into mu_out.  All pointers are device pointers:
 *   X [n][2] points; mu [k][2] centres; mu_out [k][2]; labels [n] (int32, out); stats [2] = {inertia, shift};
 *   status [2] (int32) = {0 or which bound stopped the assignment, unit augmentations made}.
 * Costs: c_ij = (x_i - mu_jx)^2 + (y_i - mu_jy)^2 in float64, every operation rounded once (no fused multiply-add).
 * The E-step works on q_ij = rint(c_ij 2^s) as 64-bit integers, s = 52 - e where max c = f 2^e, 0.5 <= f < 1 (s = 0
 * when max c = 0): one binary grid of spacing at most max c 2^-51, on which path sums are exact, so that the cycles of
 * exact weight 0 that duplicated points produce cannot round to negative ones.  The labels are an exact optimum for
 * q (successive shortest paths, one unit at a time, from the nearest-centre assignment, lowest index on every tie;
 * csrc/kmeans.hip), hence within n max c 2^-51 of the optimum for c.  inertia = sum_i c_i,labels[i].
 * Every loop of the kernels is bounded (augmentations <= n, Bellman-Ford rounds <= k + 1); a bound hit -- which the
 * method rules out -- writes status[0] != 0 and stops, and mu_out is then meaningless.
 * 1 <= k <= 1023, k <= n, n k < 2^31 (STDADK_E_ARG / STDADK_E_SHAPE), 1 <= lo <= hi, lo k <= n <= hi k
 * (STDADK_E_SHAPE).  Outputs must not alias inputs, each other or the workspace (STDADK_E_ARG).  Deterministic (no
 * float atomics, fixed orders).  Workspace: stdadk_kmeans_workspace_bytes(n, k) (0 = bad sizes), 8-byte aligned.  No
 * host read of device memory, no allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
size_t stdadk_kmeans_workspace_bytes(int64_t n, int32_t k);
int stdadk_kmeans_balanced_iter_f64(const double *X, int64_t n, int32_t k, const double *mu, int32_t lo, int32_t hi,
                                    double *mu_out, int32_t *labels, double *stats, int32_t *status, void *workspace,
                                    size_t workspace_bytes, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * k-means++ seeding for the gmm and kmeans_balanced knot initialisers (added under ABI 10: new entry points only, so
 * STDADK_ABI_VERSION stays 10): `runs` independent runs of sklearn's greedy k-means++ (_kmeans_plusplus, unit sample
 * weights) in two dimensions, entirely in float64.  The random stream does not depend on the data, so the caller draws
 * it in advance; this call does the data-dependent part.  All pointers are device pointers:
 *   X [n][2] points; first [runs] (int32) each run's first seed row, clamped to [0, n); u [runs][k-1][L] uniforms in
 *   [0, 1); idx_out [runs][k] (int32) the chosen seed rows; pot_out [runs] each run's final potential.
 * Distances are direct, every operation rounded once (no fused multiply-add):
 *   d_i = min over the chosen centres of (x_i0 - c0)^2 + (x_i1 - c1)^2; a point equal to a chosen centre has d_i == 0
 *   exactly; pot = sum_i d_i.
 * One step, for c = 1 .. k-1:
 *   thresholds   r_j = u[c-1][j] pot,  j = 0 .. L-1
 *   candidates   cand_j = the smallest i with P_i >= r_j, where P_i = d_0 + ... + d_i; n - 1 when there is none
 *   potentials   pot_j = sum_i min(d_i, |x_i - x_cand_j|^2)
 *   choice       the candidate with the smallest pot_j, the lowest j on ties: its row is idx_out[c], its minima become
 *                d and its pot_j becomes pot
 * P_i, pot and pot_j are sums of non-negative terms in one fixed order of the kernel's choosing (csrc/kmeanspp.hip:
 * chunks of rows, 32 chunks to a group, 32 groups, each level added left to right); P_i is non-decreasing in i, P_n-1
 * is pot bit for bit, and the order does not depend on j, so that two candidates with the same coordinates get the
 * same pot_j.  A pick can differ from the one strict left-to-right sums give only where rounding decides it: r_j within
 * the rounding of a prefix sum, or two candidates whose pot_j differ by less than the rounding of the sums (mutually
 * nearest candidates tie in exact arithmetic; frequent only when k nears the number of distinct points).  With pot == 0 (every point on a chosen centre) every r_j is 0 and the pick is row 0; outputs stay
 * finite and every loop has a fixed trip count.
 * 1 <= n < 2^31, 1 <= k <= min(n, 65536), 1 <= runs <= 64, 1 <= L <= 16 (STDADK_E_ARG); k == 1 reads no u (u may be
 * NULL).  X, u, pot_out and the workspace 8-byte aligned, first and idx_out 4-byte aligned (STDADK_E_ALIGN).  Outputs
 * must not alias the inputs, each other or the workspace (STDADK_E_ARG).  One workgroup per run, no atomics, nothing
 * waits on another workgroup; deterministic: the same call gives the same bits.  Up to n = 10 240 the points and d stay
 * in registers; beyond that d lives in the workspace (any n gives correct results, only the register path is fast).
 * Workspace: stdadk_kmeanspp_workspace_bytes(n, k, runs) (0 = bad sizes; STDADK_E_WORKSPACE).  No host read of device
 * memory, no allocation, capturable.
 * ------------------------------------------------------------------------------------------ */
size_t stdadk_kmeanspp_workspace_bytes(int64_t n, int32_t k, int32_t runs);
int stdadk_kmeanspp_f64(const double *X, int64_t n, int32_t k, int32_t runs, int32_t L, const int32_t *first,
                        const double *u, int32_t *idx_out, double *pot_out, void *workspace, size_t workspace_bytes,
                        stdadk_stream_t stream);

/* A10 on a site x time prediction grid (the dense inference callers loop over time slices with the SAME S
 * sites in each, scripts/train_st_interp.py:1091-1107,1232-1248,1378-1409).  Layer 0's pre-activation of row
 * (ti, s) is  sum_k phi_k(s) W0^T[p+k,:]  +  sum_j psi_j(t_ti) W0^T[p+Ks+j,:]  +  b0 : a per-site row plus a per-time
 * row, so the basis evaluation and the W0^T gather are done once per site instead of once per (site, time):
 *   stdadk_spatial_partial_f32   sp[S][h0]  (window path, fixed grid knots, p = 0; workspace as for a forward of S rows)
 *   stdadk_temporal_partial_f32  tp[T][h0]
 *   stdadk_forward_parts_f32     y_pred[T*S][Q], rows time-major: z0 = sp[row % S] + tp[row / S] + b0, then
 *                                LayerNorm/ReLU of layer 0, the remaining layers and the output layer (eval mode)
 * Same sums as stdadk_forward_f32 in another order of addition (agreement to fp32 rounding, tested).
 * All three need the first weight stored (in,out) (STDADK_FLAG_W0_T).
 * stdadk_forward_parts_supported (added under ABI 10: a new entry point only): 1 when stdadk_forward_parts_f32 runs
 * this MLP (at least one hidden layer, every hidden width a multiple of 16 up to 256, out_dim <= 8), else 0; a
 * caller that gets 0 expands the rows and calls stdadk_forward_f32. */
int32_t stdadk_forward_parts_supported(const stdadk_mlp_desc *mlp);
int stdadk_spatial_partial_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                               const stdadk_mlp_tensors *params, const float *coords, int64_t S, float *out,
                               void *workspace, size_t workspace_bytes, int32_t flags, stdadk_stream_t stream);
int stdadk_temporal_partial_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                                const stdadk_mlp_tensors *params, const float *t_values, int64_t T, float *out,
                                int32_t flags, stdadk_stream_t stream);
int stdadk_forward_parts_f32(const stdadk_mlp_desc *mlp, const stdadk_mlp_tensors *params, const float *sp,
                             int64_t S, const float *tp, int64_t T, float *y_pred, stdadk_stream_t stream);

/* A0, window path: the batch-preparation half of the step on its own — gathers rows idx[b] (NULL = rows
 * 0..B-1) of coords_all / t_all / X_all / y_all [N, y_cols] and bins them into `workspace`, exactly as
 * the step entry points would.  Software pipelining: call it for batch k+1 on a second stream (and a
 * second workspace) while step k runs, then run step k+1 with STDADK_FLAG_PREBINNED.  The caller
 * orders the streams (the workspace must not be in use by an unfinished step). */
int stdadk_bin_batch_f32(const stdadk_basis_desc *basis, const stdadk_mlp_desc *mlp,
                         const float *coords_all, const float *t_all, const float *X_all,
                         const float *y_all, const int64_t *idx, int64_t B, int32_t y_cols,
                         void *workspace, size_t workspace_bytes, int32_t flags,
                         stdadk_stream_t stream);

/* A0  batch producer (scripts/train_st_interp.py:413-460 dataset + collate, :609-612 H2D): rows
 * idx[b] (int64) of the device-resident observation arrays into contiguous batch buffers, one launch.
 * coords [N,2], t [N], y [N,Q], X [N,p] (NULL when p == 0). */
int stdadk_gather_batch_f32(const float *coords, const float *t, const float *y, const float *X,
                            const int64_t *idx, int64_t B, int32_t Q, int32_t p, float *coords_out,
                            float *t_out, float *y_out, float *X_out, stdadk_stream_t stream);

/* Integer bookkeeping of the window path, exposed for bit-exact tests:
 *   stdadk_bin_obs_f32: cell key of every observation (cx*G+cy, cx = clamp(floor(x*G),0,G-1)),
 *     cell_start[G*G+1] (first sorted position of every cell) and perm[B] (sorted position ->
 *     original index; row-major cells, ascending original index inside a cell).
 *   stdadk_knot_windows_i32: per observation and level the first knot (ix0, iy0) of the window
 *     [floor(x*(side-1))-2, +6) clamped into the grid, and its feature column
 *     col0 = p + level_offset + ix0*side + iy0.  Arrays are [B, n_levels] int32. */
size_t stdadk_bin_workspace_bytes(int64_t B, int32_t G);
int stdadk_bin_obs_f32(const float *coords, int64_t B, int32_t G, int32_t *keys,
                       int32_t *cell_start, int32_t *perm, void *workspace, size_t workspace_bytes,
                       stdadk_stream_t stream);
int stdadk_knot_windows_i32(const float *coords, int64_t B, const int32_t *sides_host,
                            int32_t n_levels, int32_t p, int32_t *ix0, int32_t *iy0, int32_t *col0,
                            stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The fp32 MFMA GEMM the Linear layers are built from (nn.Linear forward / autograd backward:
 * st_interp.py:660,689), exposed so that tests and the roofline measurement can drive it directly.
 *   C[M,N] (+bias[N]) = sum_k Aop[m][k] * Bop[k][n]
 *   a_km == 0: Aop[m][k] = A[m*lda + k]      a_km != 0: Aop[m][k] = A[k*lda + m]
 *   b_km == 0: Bop[k][n] = B[n*ldb + k]      b_km != 0: Bop[k][n] = B[k*ldb + n]
 * (a_km != 0 with b_km == 0 is not built.)  workspace: stdadk_gemm_workspace_bytes(M,N,K) bytes
 * of split-K slab space (may be 0 / NULL when the shape does not split).
 * ------------------------------------------------------------------------------------------ */
size_t stdadk_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K);

int stdadk_gemm_f32(const float *A, int64_t lda, int32_t a_km, const float *B, int64_t ldb,
                    int32_t b_km, int32_t M, int32_t N, int32_t K, const float *bias, float *C,
                    int64_t ldc, void *workspace, size_t workspace_bytes, stdadk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Measurement aid: when enabled, every kernel the library launches is bracketed by two HIP events
 * on its launch stream.  stdadk_profile_collect synchronises them and writes one "name\tms\n" line
 * per launch (launch order) into buf; it returns the bytes needed including the terminator (call
 * again with a bigger buffer if that exceeds cap).  Enabling clears earlier records.  Not for use
 * under stream capture; host-side, single-threaded.  In a dry run (STDADK_DRY_RUN=1) nothing is launched or timed,
 * but the names are still recorded: the lines read "name\t0.000000" -- the launch chain of a call without a device.
 * ------------------------------------------------------------------------------------------ */
int stdadk_profile_enable(int32_t on);
int64_t stdadk_profile_collect(char *buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* STDADK_H */
