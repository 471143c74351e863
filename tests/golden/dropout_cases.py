"""Training steps with GENERATED dropout masks against float64: the models of tests/golden/shape_cases.py with dropout
switched on, shared by tests/test_dropout_cases_cpu.py (runs anywhere) and tests/test_gpu_dropout.py.  The masks of
the reference come from oracle/dropout.py, the CPU restatement of the contract in include/stdadk.h.

The keep decision is written out in four places of the library (drop_keep in common.h for the per-layer kernels,
l1_row_epilogue in l1_body.h, ln_fwd_rows and ln_bwd_rows in tail_body.h); CASES names what each case reaches.
"""
import numpy as np

from golden import cases
from golden import shape_cases as SC
from golden import site_cases
from oracle import dropout as drp
from oracle import stdadk_oracle as orc

TOL = 1e-5                   # the project's bound (test_gpu_mlp_shapes.py), kept
KINK_TOL = 1e-6
MAX_NEAR_KINK = 2            # 300-row cases, as test_gpu_mlp_shapes.py; the larger batches get no cap on the count

CASES = {
    # window path: layer 0 in l1_row_epilogue (column CPL * lane + c, SORTED row), later layers in the tail's
    # ln_fwd_rows / ln_bwd_rows (one hash per column pair lane + 128 pp, + 64; CC = ceil(width / 64) columns per lane)
    "w_depth1": "window: the layer-0 epilogue only, H = 256, CPL = 4",
    "w_k48_q2": "window: H = 128, CPL = 2; tail width 48: CC = 1, the second half of the pair is absent",
    "w_k80_k176_noln": "window: widths 80 and 176: CC = 2 and CC = 3, the odd CC leaves the last pair half empty; "
                       "no LayerNorm",
    "w_depth8_q8": "window: layer_id 0..7",
    # materialising path, caller rows
    "d_D256": "dense: layer 0 inside the tail launch",
    "d_D513": "dense: layer 0 outside the tail launch (ln_relu_fwd_kernel / drop_keep), then the tail",
    # per-layer kernels of mlp.hip (drop_keep)
    "g_h40_24": "per-layer: widths that are no multiple of 64",
    "g_h320_72_q3": "per-layer: a width above 256 (pair index >= 128)",
}
WINDOW_CASES = [k for k in CASES if k.startswith("w_")]

# p = 0.1 is the shipped value (threshold 6554); 0.25 and 0.5 make p * 65536 integral (16384, 32768); 1e-5 gives
# threshold 1: an element is dropped only when its 16 bits are 0
P_SHIPPED = 0.1
P_EXTRA = (0.25, 0.5, 1e-5)
P_EXTRA_CASES = ("w_k80_k176_noln", "g_h40_24")
THRESHOLDS = {0.1: 6554, 0.25: 16384, 0.5: 32768, 1e-5: 1}

# 300 rows: 16-row tiles with a ragged one of 12, the one-launch step kernel; BIG_B: the separate window and tail
# kernels; ROWS32_B / ROWS64_B: RPW > 1 in the tail's row phases, grow = row0 + RPW * wave + rr
SMALL_B = 300
LARGE = [("w_k80_k176_noln", SC.BIG_B), ("w_depth8_q8", SC.BIG_B), ("w_k80_k176_noln", SC.ROWS32_B),
         ("w_k80_k176_noln", SC.ROWS64_B)]

# 2^62 - 1 is the top of the range torch.randint(0, 2 ** 62) can draw
SEEDS = (5, 123456789012345, 2 ** 62 - 1)

# (case, B, p); entry i takes SEEDS[i % 3] as its TrainStep seed and i as the torch.manual_seed of its module run
ENTRIES = [(n, SMALL_B, P_SHIPPED) for n in CASES] + [(n, SMALL_B, p) for n in P_EXTRA_CASES for p in P_EXTRA] \
    + [(n, B, P_SHIPPED) for n, B in LARGE]

# input seeds moved off the case's own where a float64 run with masks puts more than MAX_NEAR_KINK units within
# KINK_TOL of a ReLU kink (tests/test_dropout_cases_cpu.py asserts the count): {(case, B, p): input seed}
INPUT_SEED = {("w_k80_k176_noln", SMALL_B, 0.1): 20103, ("w_k80_k176_noln", SMALL_B, 0.5): 20103}

STEPS = 3                    # consecutive one-call steps of test_gpu_dropout.py (c)
ADAM_EPS = 1e-3              # test_gpu_round2._DP_EPS: keeps the update linear in rounding-level gradients
RANK_ENTRY, RANK_BASE_SEED = 1, SEEDS[1]      # test_gpu_dropout.py (d): ranks 0 and 1 of 2 on ENTRIES[1]
CLIP_OF_NORM = 0.5           # grad_clip = half the reference norm of step 0: clipping active


def entry_id(e):
    return f"{e[0]}-{e[1]}-p{e[2]:g}"


def entry_seed(e):
    return SEEDS[ENTRIES.index(e) % len(SEEDS)]


def config(e):
    """shape_cases.config of the entry with `dropout` added."""
    name, B, p = e
    cfg = SC.config(name, None if B == SMALL_B else B)
    if e in INPUT_SEED:
        cfg["input_seed"] = INPUT_SEED[e]
    cfg["dropout"] = p
    return cfg


def row_keys(coords, window):
    """Row key of every caller row: its own index on the materialising path, its position in the cell-sorted batch
    on the window path (the permutation test_bin_obs_bit_exact pins)."""
    B = len(coords)
    if not window:
        return np.arange(B, dtype=np.int64)
    return drp.window_rows(coords, site_cases.pick_cell_grid(B))


def masks(cfg, seed, step, rows):
    return drp.keep_masks(seed, step, rows, cfg["hidden_dims"], cfg["dropout"])


def reference(cfg, inp, params, seed, step, window, kink_tol=KINK_TOL):
    """float64 (y, loss, grads, alts) of one step with the replica's masks."""
    X, coords, t, y = inp
    mk = masks(cfg, seed, step, row_keys(coords, window))
    return orc.train_step_grads(X, coords, t, y, params, cfg, kink_tol=kink_tol, drop_masks=mk, drop_p=cfg["dropout"])


# ------------------------------------------------------------------------------------------------ comparison
def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def compare(got_y, got_loss, got_grads, ref, max_alts=MAX_NEAR_KINK, tol=TOL):
    """One step against its float64 reference (y, loss, grads, alts): y max-abs over max(1, max|y|) (skipped when
    got_y is None), loss relative, every gradient tensor rel-L2 after orc.fit_kink_sides, each <= tol; at most
    `max_alts` near-kink units (None: no cap).  Returns dict(y, loss, worst, worst_key, near, flipped)."""
    yo, lo, go, alts = ref
    e_y = 0.0
    if got_y is not None:
        gy = np.asarray(got_y, np.float64)
        assert gy.shape == yo.shape, ("y shape", gy.shape, yo.shape)
        e_y = float(np.abs(gy - yo).max() / max(1.0, float(np.abs(yo).max())))
    e_l = abs(float(got_loss) - lo) / lo
    gg = {k: np.asarray(v, np.float64) for k, v in got_grads.items()}
    assert set(gg) == set(go), (sorted(gg), sorted(go))
    for k in go:
        assert gg[k].shape == go[k].shape and np.isfinite(gg[k]).all(), k
    flipped, adj = orc.fit_kink_sides(gg, go, alts)
    errs = {k: rel_l2(gg[k], adj[k]) for k in go}
    worst = max(errs, key=errs.get)
    out = dict(y=e_y, loss=e_l, worst=errs[worst], worst_key=worst, near=len(alts), flipped=flipped, adjusted=adj)
    print(f"    y {e_y:.2e} loss {e_l:.2e} worst gradient rel-L2 {errs[worst]:.2e} ({worst}); {len(alts)} units within "
          f"{KINK_TOL} of a kink, flipped {len(flipped)}: {flipped}")
    assert e_y <= tol, ("y", e_y)
    assert e_l <= tol, ("loss", e_l)
    assert len(flipped) <= len(alts) and (max_alts is None or len(alts) <= max_alts), (flipped, len(alts))
    for k, e in errs.items():
        assert e <= tol, (k, e)
    return out
