"""Shape matrix of the fused MLP tail (csrc/tail_body.h), the dense layer 0 inside the tail launch and the
per-layer fallback (csrc/mlp.hip): widths, depths and heads that tail_supported() accepts (or just refuses) and
that no golden vector of the reference covers.  Data only: `cases.MODEL_CASES`-style dicts, so that
cases.make_inputs / cases.make_state / test_gpu_parity.build_model apply unchanged.  The float64 reference of
every case is the numpy oracle (checked against its torch restatement in tests/test_shape_cases_cpu.py).

All cases: Wendland basis unless stated, 300 rows (18 full 16-row tiles and a ragged one of 12), dropout 0.

What each case reaches (K = a GEMM's reduction width, N = its output width; the fp32 K loop walks 32-deep
chunks, the bf16 one 64-deep chunks):
  w_depth1           n_layers == 0: the launch is input tile + head only
  w_k48_q2           forward K = 128 (unrolled) into N = 48; backward dA with K = 48 (2 chunks, ragged half) from
                     the [K][N] layout; head Q = 2; bf16 K % 64 = 48
  w_k80_k176_noln    forward K = 80 (3 chunks, ragged) and K = 176 -> head; backward K = 176 (6 chunks, ragged)
                     and K = 80; no LayerNorm; bf16 K % 64 = 16 and 48
  w_narrow_wide_q4   128 -> 16 -> 240 -> 32: one wave of sixteen has an N tile, then fifteen; K = 16 (a single
                     half chunk), K = 240 (8 chunks, ragged), K = 32; head Q = 4
  w_depth8_q8        STDADK_MAX_HIDDEN layers, K = 208, 144, 112, 96, 64, 48, 16 in both directions (7, 5, 4, 3,
                     2, 2, 1 chunks: odd and even counts of the double-buffered loop); head Q = 8 = TAIL_MAXQ
  d_D256 .. d_D513   layer 0 inside the tail launch (TailDense0): D = 256 fits one LDS half, 257 needs the second,
                     512 is the last inside the launch, 513 the first outside (rbf_build + GEMM)
  d_gauss_q2         the same with the Gaussian basis, K = 112 / 144, Q = 2
  g_*                widths the tail refuses (not a multiple of 16, wider than 256): the per-layer LayerNorm /
                     ReLU / GEMM / head kernels of mlp.hip

Rows per workgroup: tail_rows() (csrc/tail.hip) gives 64-row tiles once ceil(B / 64) >= 256, else 32-row tiles once
ceil(B / 32) >= 256, else 16.  At 300 and 4 097 rows that is 16: only the MT = 1 instantiations meet the rolled K
loop with its ragged last chunk.  ROWS32_B = 255 * 32 + 1 = 8 161 is the smallest batch with 32-row tiles (MT = 2:
255 full tiles and one of a single row), ROWS64_B = 255 * 64 + 1 = 16 321 the smallest with 64-row tiles (MT = 4,
likewise); BIG_CASES run at both.
"""
import numpy as np

from . import cases

_COMMON = dict(p=0, k_temporal_centers=[10, 15], basis="wendland", output_dim=1, layernorm=True, B=300)
_WINDOW = dict(_COMMON, k_spatial_centers=[144, 400])          # D = 569; window path with hidden[0] in {128, 256}


def _c(base, **kw):
    return dict(base, **kw)


SHAPE_CASES = {
    # ---- window path
    "w_depth1": _c(_WINDOW, hidden_dims=[256], seed=101),
    "w_k48_q2": _c(_WINDOW, hidden_dims=[128, 48], output_dim=2, seed=102),
    "w_k80_k176_noln": _c(_WINDOW, hidden_dims=[256, 80, 176], layernorm=False, seed=103),
    "w_narrow_wide_q4": _c(_WINDOW, hidden_dims=[128, 16, 240, 32], output_dim=4, seed=104),
    "w_depth8_q8": _c(_WINDOW, hidden_dims=[256, 208, 144, 112, 96, 64, 48, 16], output_dim=8, seed=105),
    # ---- materialising path, one knot level, temporal list chosen to hit D exactly
    "d_D256": _c(_COMMON, k_spatial_centers=[225], k_temporal_centers=[10, 21], hidden_dims=[48, 80], seed=111),
    "d_D257_depth1": _c(_COMMON, p=1, k_spatial_centers=[225], k_temporal_centers=[10, 21], hidden_dims=[16],
                        seed=112),
    "d_D512": _c(_COMMON, k_spatial_centers=[484], k_temporal_centers=[13, 15], hidden_dims=[240, 16, 112],
                 seed=113),
    "d_D513": _c(_COMMON, p=1, k_spatial_centers=[484], k_temporal_centers=[13, 15], hidden_dims=[80, 48],
                 seed=114),
    "d_gauss_q2": _c(_COMMON, k_spatial_centers=[225], k_temporal_centers=[10, 21], hidden_dims=[112, 144],
                     basis="gaussian", output_dim=2, seed=115),
    # ---- no tail: the per-layer kernels
    "g_h40_24": _c(_WINDOW, hidden_dims=[40, 24], seed=121),
    "g_h40_24_noln": _c(_WINDOW, hidden_dims=[40, 24], layernorm=False, seed=122),
    "g_h320_72_q3": _c(_WINDOW, hidden_dims=[320, 72], output_dim=3, seed=123),
}

WINDOW_CASES = [k for k in SHAPE_CASES if k.startswith("w_")]
DENSE0_CASES = [k for k in SHAPE_CASES if k.startswith("d_")]
FALLBACK_CASES = [k for k in SHAPE_CASES if k.startswith("g_")]

# feature widths the d_* cases are named after
FEATURE_WIDTH = {"d_D256": 256, "d_D257_depth1": 257, "d_D512": 512, "d_D513": 513, "d_gauss_q2": 256}

# the first batch past the one-launch step kernel (l1_tail_supported: B <= 4096): separate tail kernels, a ragged
# last tile of one row
BIG_B = 4097
BIG_CASES = ["w_k80_k176_noln", "w_depth8_q8"]
ROWS32_B = 255 * 32 + 1      # smallest batch with 32-row tail tiles
ROWS64_B = 255 * 64 + 1      # smallest batch with 64-row tail tiles


def config(name, B=None):
    """The case's dict; with `B` the same model on another batch size (its own input seed; the parameters keep
    the case's seed, cases.make_state reads seed + 1000)."""
    cfg = dict(SHAPE_CASES[name])
    if B is not None and B != cfg["B"]:
        cfg["B"] = B
        cfg["input_seed"] = cfg["seed"] + B
    return cfg


def make_inputs(cfg):
    """cases.make_inputs, with (B, Q) standard-normal targets where the head has more than one output."""
    X, coords, t, y = cases.make_inputs(dict(cfg, seed=cfg.get("input_seed", cfg["seed"])))
    Q = cfg["output_dim"]
    if Q > 1:
        y = np.random.RandomState(cfg.get("input_seed", cfg["seed"])).standard_normal((cfg["B"], Q)).astype(np.float32)
    return X, coords, t, y
