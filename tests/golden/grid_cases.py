"""Site x time prediction grids (Predictor.predict_grid / score_grid, stnf.utils.grid_scores, predict_all_times)
against the float64 oracle: models, grids, sites and times, shared by tests/test_grid_cases_cpu.py (runs anywhere)
and tests/test_gpu_predict_grid.py.  Data only: numpy, seeded RandomState (MT19937), dicts in the style of
cases.MODEL_CASES / shape_cases.SHAPE_CASES.  Every model has p = 0 (the covariate refusal is pinned elsewhere).

ROUTES.  Predictor._grid_chunks takes one of three, recorded per model as `route`:
  window         fixed knots on the window path: stdadk_spatial_partial_f32 once per `chunk` sites (its own binning,
                 l1_window_forward with raw = 1, un-permutation into sp[s0:s0+n])
  materialising  first weight stored (in,out) but no window path for the sites (learnable knots, Gaussian basis,
                 small tables, engine-owned storage): rbf_build + one GEMM with the first k_spatial rows of W0^T
  expanded       an MLP stdadk_forward_parts_f32 refuses: every chunk's rows expanded, through predict()
The first two end in stdadk_temporal_partial_f32 and one stdadk_forward_parts_f32 per chunk of time slices.

TILES.  tail_rows() (csrc/tail.hip) picks the rows per workgroup from the rows of ONE forward_parts call, n S:
64 once ceil(rows / 64) >= 256 (16 321 rows), else 32 once ceil(rows / 32) >= 256 (8 161 rows), else 16; bf16
operands stop at 32.  Global row g of a tile reads sp[g % S] and tp[g / S]; with S prime no tile boundary falls on a
slice boundary.

ONE CONDITION, asserted for every case by tests/test_grid_cases_cpu.py: no library call sees more than
site_cases.MAX_ROWS_PER_CELL rows in one binning cell.  On the window route spatial_partial bins the sites of its
call; the materialising route bins nothing; on the expanded route predict() bins the expanded rows, n copies of every
site per chunk of n slices, so those cases stay at S T = 67 x 7 and below, and S == 1 with many times appears on
the parts routes only.

The float64 reference of a case with 16 336 rows and 544 knots is 71 MB per intermediate; of the C2 table (10 304
knots) it would be 1.3 GB, so the C2 models stay at or below about 1 000 rows.
"""
import numpy as np

from golden import cases
from golden import shape_cases as SC
from golden import site_cases as sc
from oracle import stdadk_oracle as orc

TOL = sc.TOL                 # max|y - y64| <= TOL max(1, max|y64|): test_gpu_mlp_shapes.TOL, site_cases.TOL

_227 = dict(p=0, k_spatial_centers=[25, 81, 121], k_temporal_centers=[10, 15, 45], layernorm=True, basis="wendland",
            output_dim=1, B=0)
_C2 = cases.MODEL_CASES["c2_b257"]


def _m(cfg, route, kind="plain", force_window=True, engine=False, learn=None, scattered=None):
    """One model: `cfg` a MODEL_CASES-style dict (parameters from cases.make_state), `kind` plain / delta / learn /
    scattered, `force_window` the model's force_window_path, `engine` a TrainStep constructed on it first."""
    return dict(cfg=cfg, route=route, kind=kind, force_window=force_window, engine=engine, learn=learn,
                scattered=scattered)


# scattered fixed knots: the table test_gpu_round2 builds for its grid check (_scattered_model([1024, 4096],
# "triangular", False, 80): random_site knots, three pushed outside the unit square, two inflated bandwidths)
SCATTERED = dict(sizes=[1024, 4096], basis="triangular", seed=80, hidden=(256, 128))

MODELS = {
    # ---- window route, fixed grid knots ([144, 400]: 544 knots, D = 569)
    "w_depth1": _m(SC.SHAPE_CASES["w_depth1"], "window"),
    "w_k48_q2": _m(SC.SHAPE_CASES["w_k48_q2"], "window"),
    "w_k80_k176_noln": _m(SC.SHAPE_CASES["w_k80_k176_noln"], "window"),
    "w_narrow_wide_q4": _m(SC.SHAPE_CASES["w_narrow_wide_q4"], "window"),
    "w_depth8_q8": _m(SC.SHAPE_CASES["w_depth8_q8"], "window"),
    "w_tri": _m(dict(SC._WINDOW, hidden_dims=[256, 128], basis="triangular", seed=131), "window"),
    "w_kt1": _m(dict(SC._WINDOW, k_temporal_centers=[1], hidden_dims=[128, 64], seed=132), "window"),
    "c2_b257": _m(_C2, "window"),
    # ---- window route, scattered fixed knots
    "s_tri": _m(dict(p=0, k_spatial_centers=SCATTERED["sizes"], k_temporal_centers=[10, 15],
                     hidden_dims=list(SCATTERED["hidden"]), layernorm=True, basis=SCATTERED["basis"], output_dim=1,
                     B=0, seed=SCATTERED["seed"]), "window", kind="scattered", scattered=SCATTERED),
    # ---- materialising route
    "d_D256": _m(SC.SHAPE_CASES["d_D256"], "materialising"),
    "d_D512": _m(SC.SHAPE_CASES["d_D512"], "materialising"),                 # K = 484, h0 = 240
    "d_gauss_q2": _m(SC.SHAPE_CASES["d_gauss_q2"], "materialising"),
    "default227_delta5": _m(cases.quantile_cfg("default227_delta5")[0], "materialising", kind="delta",
                            force_window=False),
    "default227_learn": _m(cases.learn_cfg("default227_learn")[0], "materialising", kind="learn", force_window=False),
    "c2_b257_learn": _m(cases.learn_cfg("c2_b257_learn")[0], "materialising", kind="learn"),     # K = 10 304
    "d_gauss_q2_engine": _m(SC.SHAPE_CASES["d_gauss_q2"], "materialising", engine=True),  # W0 an engine-owned .t() view
    # ---- widths and heads the tail refuses: expanded rows through predict()
    "r_227_h40_24": _m(dict(_227, hidden_dims=[40, 24], seed=141), "expanded", force_window=False),
    "r_227_h320_72": _m(dict(_227, hidden_dims=[320, 72], seed=142), "expanded", force_window=False),
    "r_227_q9": _m(dict(_227, hidden_dims=[48], output_dim=9, seed=143), "expanded", force_window=False),
    "r_w_h256_24": _m(dict(SC._WINDOW, hidden_dims=[256, 24], seed=144), "expanded"),
    "r_w_h128_320": _m(dict(SC._WINDOW, hidden_dims=[128, 320], seed=145), "expanded"),
    "r_c2_q9": _m(dict(_C2, output_dim=9, seed=146), "expanded"),                 # the shipped C2 knots, nine quantiles
}
REFUSED = [k for k, v in MODELS.items() if v["route"] == "expanded"]


# ------------------------------------------------------------------------------------------------ knots
def learn_knots(cfg):
    """(centers (Ks,2), log_bw (Ks,)) float32 of a learnable model: the uniform grid moved by cases.knot_perturbation,
    both sums in float32."""
    cen, bw, _ = orc.uniform_knots(cfg["k_spatial_centers"])
    dc, dlb = cases.knot_perturbation(cfg)
    return (cen + dc).astype(np.float32), (np.log(bw).astype(np.float32) + dlb).astype(np.float32)


def knots(name, model=None):
    """(centers, bandwidths) of model `name` as float64 arrays of its float32 values.  Scattered knots are not data
    here (the initialiser draws them): they are read from the built `model`."""
    spec = MODELS[name]
    if spec["kind"] == "scattered":
        sb = model.spatial_basis
        return (sb.centers.detach().cpu().numpy().astype(np.float64),
                sb.bandwidths.detach().cpu().numpy().astype(np.float64))
    if spec["kind"] == "learn":
        cen, lbw = learn_knots(spec["cfg"])
        return cen.astype(np.float64), np.exp(lbw.astype(np.float64))
    cen, bw, _ = orc.uniform_knots(spec["cfg"]["k_spatial_centers"])
    return cen.astype(np.float64), bw.astype(np.float64)


def params64(name):
    """float64 parameters {mlp.*} of model `name` (the delta head as its equivalent output layer)."""
    cfg = MODELS[name]["cfg"]
    st = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    if MODELS[name]["kind"] == "delta":
        st = orc.delta_to_standard(st, cfg)[0]
    return st


def forward64(name, coords, t, model=None, dtype=np.float64):
    """(y (N,Q), phi, psi) of rows (coords, t).  Fixed uniform knots: orc.model_forward itself; moved or scattered
    knots: the same lines with the model's own table."""
    cfg = MODELS[name]["cfg"]
    ps = params64(name)
    if dtype is not np.float64:
        ps = {k: v.astype(dtype) for k, v in ps.items()}
    t = np.asarray(t).reshape(-1, 1)
    if MODELS[name]["kind"] in ("plain", "delta"):
        y, _, phi, psi, _ = orc.model_forward(None, coords, t, ps, cfg, dtype=dtype)
        return y, phi, psi
    cen, bw = knots(name, model)
    tc, tb = orc.temporal_knots(cfg["k_temporal_centers"])
    phi = orc.spatial_basis(coords, cen, bw, cfg["basis"], dtype)
    psi = orc.temporal_basis(t, tc, tb, dtype)
    y = orc.mlp_forward(orc.features(None, phi, psi, 0), ps, len(cfg["hidden_dims"]), cfg["layernorm"], dtype)[0]
    return y, phi, psi


def grid64(name, coords, tv, model=None, dtype=np.float64):
    """(T, S, Q) reference grid: the forward on the expanded rows np.tile(coords, (T, 1)), np.repeat(tv, S)."""
    S, T = len(coords), len(tv)
    y = forward64(name, np.tile(coords, (T, 1)), np.repeat(tv, S), model, dtype)[0]
    return y.reshape(T, S, -1)


# ------------------------------------------------------------------------------------------------ sites and times
def uniform_sites(S, seed):
    return np.random.RandomState(seed).uniform(-0.05, 1.05, (S, 2)).astype(np.float32)


def listed_twice(S=130, seed=305):
    """S sites of which the last 30 repeat the first 30 exactly (a site listed twice gets the same row twice)."""
    pts = uniform_sites(S - 30, seed)
    return np.concatenate([pts, pts[:30]]).astype(np.float32)


def sites(spec, cfg):
    """spec: ("uniform", S) or the name of a site set of site_cases / "listed_twice"."""
    if isinstance(spec, tuple):
        return uniform_sites(spec[1], 900 + spec[1])
    if spec == "listed_twice":
        return listed_twice()
    return sc.site_set(spec, cfg)


def times(T, cfg, seed):
    """T float32 times in no order: 1.0 (the last temporal knot), a value below 0, an inner temporal knot (exactly),
    a value above 1, 0.0, then uniform draws from [-0.1, 1.1]; from T = 3 on the last repeats the first."""
    tc = orc.temporal_knots(cfg["k_temporal_centers"])[0]
    tv = np.random.RandomState(seed).uniform(-0.1, 1.1, T).astype(np.float32)
    special = np.array([1.0, -0.07, tc[len(tc) // 2], 1.08, 0.0], dtype=np.float32)
    tv[:min(T, 5)] = special[:T]
    if T >= 3:
        tv[T - 1] = tv[0]
    return tv


# ------------------------------------------------------------------------------------------------ grids
def tail_rows(rows, bf16=False):
    """csrc/tail.hip tail_rows(): rows per workgroup of a forward_parts call on `rows` rows."""
    if -(-rows // 64) >= 256 and not bf16:
        return 64
    return 32 if -(-rows // 32) >= 256 else 16


def slices_per_call(S, max_rows):
    """Predictor._slices_per_call."""
    return max(1, (max_rows or (1 << 30)) // max(S, 1))


def _g(model, sites_spec, T, chunk, max_rows, reaches):
    return dict(model=model, sites=sites_spec, T=T, chunk=chunk, max_rows=max_rows, reaches=reaches)


U = "uniform"
CASES = {
    # ---- 32- and 64-row tiles, S = 1021 prime: every tile boundary inside a time slice
    "w_depth1-1021x8": _g("w_depth1", (U, 1021), 8, 4096, None, "32-row tiles, head only"),
    "w_k48_q2-1021x16": _g("w_k48_q2", (U, 1021), 16, 4096, None, "64-row tiles, Q = 2"),
    "w_depth8_q8-1021x16": _g("w_depth8_q8", (U, 1021), 16, 4096, None, "64-row tiles, depth 8, Q = 8"),
    "w_tri-1021x8": _g("w_tri", (U, 1021), 8, 4096, None, "32-row tiles, triangular basis"),
    "d_D512-1021x8": _g("d_D512", (U, 1021), 8, 4096, None, "32-row tiles at h0 = 240"),
    "d_gauss_q2-1021x16": _g("d_gauss_q2", (U, 1021), 16, 4096, None, "64-row tiles, Gaussian basis, Q = 2"),
    "d_gauss_q2_engine-1021x8": _g("d_gauss_q2_engine", (U, 1021), 8, 4096, None, "32-row tiles, engine-owned W0"),
    # ---- a last tile of one row
    "w_k80_k176_noln-859x19": _g("w_k80_k176_noln", (U, 859), 19, 4096, None, "16 321 rows: 64-row tiles, last of 1"),
    "d_D512-859x19": _g("d_D512", (U, 859), 19, 4096, None, "16 321 rows at h0 = 240"),
    "w_narrow_wide_q4-8161x1": _g("w_narrow_wide_q4", (U, 8161), 1, 8192, None, "T == 1: g / S == 0 everywhere"),
    "w_narrow_wide_q4-1x8161": _g("w_narrow_wide_q4", "single_site", 8161, 4096, None, "S == 1: every row another time"),
    "default227_learn-1x8161": _g("default227_learn", "single_site", 8161, 4096, None, "S == 1, learnable knots"),
    # ---- time chunks: tp starts at t0 > 0, a short last chunk
    "w_depth8_q8-border-x7": _g("w_depth8_q8", "border", 7, 4096, 3 * 64 + 5, "chunks of 3, 3, 1 slices; border sites"),
    "c2_b257-67x7": _g("c2_b257", (U, 67), 7, 4096, 3 * 67 + 5, "chunks of 3, 3, 1 slices, C2"),
    "c2_b257_learn-67x7": _g("c2_b257_learn", (U, 67), 7, 4096, 3 * 67 + 5, "chunks of 3, 3, 1; 10 304 moved knots"),
    "d_gauss_q2-blobs-x7": _g("d_gauss_q2", "blobs", 7, 4096, 3 * 300 + 5, "chunks of 3, 3, 1 slices; clustered sites"),
    "w_kt1-on_knots-x7": _g("w_kt1", "on_knots", 7, 4096, 3 * 200 + 5, "one temporal knot; sites on knots"),
    "w_k80_k176_noln-1021x11": _g("w_k80_k176_noln", (U, 1021), 11, 4096, 8 * 1021,
                                  "chunks of 8 and 3 slices: 32-row tiles, then 16-row tiles"),
    "default227_delta5-1021x11": _g("default227_delta5", (U, 1021), 11, 4096, 8 * 1021,
                                    "delta head, Q = 5; 32-row, then 16-row tiles"),
    # ---- site chunks
    "w_k48_q2-1003x3-chunk64": _g("w_k48_q2", (U, 1003), 3, 64, None, "16 spatial_partial calls, the last of 43 sites"),
    "c2_b257-331x3-chunk64": _g("c2_b257", (U, 331), 3, 64, None, "6 spatial_partial calls on C2, the last of 11"),
    "w_tri-blobs-x7-chunk128": _g("w_tri", "blobs", 7, 128, 3 * 300 + 5, "3 site calls (128, 128, 44) x chunks 3, 3, 1"),
    "s_tri-509x7-chunk256": _g("s_tri", (U, 509), 7, 256, 3 * 509 + 5, "scattered knots: 2 site calls x chunks 3, 3, 1"),
    "d_D256-1030x2": _g("d_D256", (U, 1030), 2, 1024, None, "materialising site step 1024 + 6"),
    # ---- sites
    "w_k48_q2-one_cell-x5": _g("w_k48_q2", "one_cell", 5, 4096, None, "five sites in one binning cell"),
    "w_depth1-listed_twice-x5": _g("w_depth1", "listed_twice", 5, 64, 2 * 130, "sites listed twice; 3 site calls"),
    "default227_learn-on_knots-x7": _g("default227_learn", "on_knots", 7, 4096, 3 * 193 + 5, "sites on the grid the knots left"),
    "default227_delta5-border-x3": _g("default227_delta5", "border", 3, 4096, None, "delta head, border sites"),
    # ---- refused widths: the expanded route (S T small: predict() bins the expanded rows)
    "r_227_h40_24-67x3": _g("r_227_h40_24", (U, 67), 3, 1024, None, "widths 40, 24"),
    "r_227_h40_24-67x7": _g("r_227_h40_24", (U, 67), 7, 1024, 3 * 67 + 5, "widths 40, 24; chunks of 3, 3, 1 slices"),
    "r_227_h320_72-67x3": _g("r_227_h320_72", (U, 67), 3, 1024, None, "widths 320, 72"),
    "r_227_q9-67x3": _g("r_227_q9", (U, 67), 3, 1024, None, "nine outputs"),
    "r_w_h256_24-67x3": _g("r_w_h256_24", (U, 67), 3, 1024, None, "window layer 0, width 24 after it"),
    "r_w_h128_320-67x3": _g("r_w_h128_320", (U, 67), 3, 1024, None, "window layer 0, width 320 after it"),
    "r_c2_q9-67x3": _g("r_c2_q9", (U, 67), 3, 1024, None, "C2 knots, nine quantiles"),
}


def inputs(case):
    """(coords (S,2), tv (T,)) float32 of a case."""
    c = CASES[case]
    cfg = MODELS[c["model"]]["cfg"]
    co = sites(c["sites"], cfg)
    return co, times(c["T"], cfg, 500 + len(co) + c["T"])


def time_chunks(case):
    """[(t0, n)] of the case's chunks of time slices."""
    c = CASES[case]
    S = len(inputs(case)[0])
    per = slices_per_call(S, c["max_rows"])
    return [(t0, min(per, c["T"] - t0)) for t0 in range(0, c["T"], per)]


def site_chunks(case):
    """[(s0, n)] of the spatial_partial calls of a window-route case (the materialising route bins nothing)."""
    c = CASES[case]
    S = len(inputs(case)[0])
    return [(s0, min(c["chunk"], S - s0)) for s0 in range(0, S, c["chunk"])]


def tile_heights(case, bf16=False):
    """Tile height of every forward_parts call of a parts-route case, in call order."""
    S = len(inputs(case)[0])
    return [tail_rows(n * S, bf16) for _, n in time_chunks(case)]


def smallest_case(model):
    """The model's case with the fewest rows."""
    own = [k for k, c in CASES.items() if c["model"] == model]
    return min(own, key=lambda k: len(inputs(k)[0]) * CASES[k]["T"])


def grid_error(got, ref):
    """The comparator: max|got - ref| / max(1, max|ref|) of two (T, S, Q) grids."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))
