"""Cases, inputs, float64 reference, bound scale and comparator of the per-knot tests of the learnable-knot gradients
(tests/test_gpu_knot_gradients.py, the CPU half in tests/test_knot_cases_cpu.py, the recorded figures of
make_knot_achieved.py).

Numpy only and deterministic (numpy.random.RandomState), like cases.py, optim_cases.py and site_cases.py: the GPU box
rebuilds every input.  Every input is a float32 array; the float64 reference (oracle.stdadk_oracle: knot_backward,
domain_penalty, movement_penalty, damping_factor, learnable_step_grads) is computed from those float32 values.

THE BOUND, per knot k and output j in (d_cx, d_cy, d_log_bw):

    |got - ref| <= K 2^-24 S[k, j]

with S in float64 the sum of the magnitudes of what is added to form the output:

  embedding level (G = dL/dphi given)
      S[k, j] = sum over the rows b that reach k of |G[b, k]| P w_j(b, k)
      P = sup |phi'| of the basis (sup_prime: found numerically), NOT |phi'(r)|: near r = 1 the float32 evaluation of
      (1 - r)^5 has an absolute error, not a relative one;
      w = |dx| / (d s), |dy| / (d s), r -- 0 for the centres at d == 0 (cdist's backward);
      a row reaches a compact-support knot when r64 < 1; every row reaches a Gaussian knot.
  step level
      |G[b, k]| is replaced by sum_h |dZ0[b, h]| |W0[h, p + k]|: G is itself a float32 sum over the hidden width, in
      either association -- G first and then per row (materialising route) or sum_b q_b dZ0[b, :] first and then the
      dot product with the knot's row of W0^T (window route).
  with a stdadk_knot_train, for the centres
      S = f_k (S_data + pen_grad_scale (dom_w |2 v| + mov_w |2 m|)),  f_k the float64 damping factor (1 when off).

S == 0 therefore means "nothing is added": the output must then be exactly 0.  K is not chosen here: it is K_FACTOR
times what a float32 restatement of the same formulas achieves against this reference (make_knot_achieved.py ->
knot_achieved.json), per output, the maximum over all cases below.  The comparator leaves no knot and no row out.

CONDITIONS the inputs keep (asserted by check_conditions / tests/test_knot_cases_cpu.py on the reference alone):
  * compact-support bases: no (row, knot) pair with |r64 - 1| <= KINK_BAND.  phi' of the triangular basis jumps there,
    and the window route drops a pair with phi == 0 where the materialising route keeps r <= 1; rows are redrawn until
    no such pair exists.  (Kept for Wendland too: a pair float32 and float64 put on different sides of the support's
    edge would give a 1e-30 where the scale says exactly 0.)
  * rows placed on knots copy the float32 centre values: d == 0 exactly.
  * every compact-support case has MIN_UNREACHED knots that no row reaches, min_b r64 > 1 + UNREACHED_MARGIN -- but
    for tables too small to hold them (Ks < 24: the Ks = 1 shape of the kernel's own tests).
  * every step case has knots below 0 and above 1 in x and in y, coordinates exactly 0.0 and exactly 1.0, a knot not
    moved at all, one moved by less than the positive damping threshold and one by more (a threshold of 0 leaves no
    room below it: that class is asserted for the settings with a positive threshold).
  * every window case has a knot reached by exactly one row and one reached by a row count that is no multiple of 8;
    with 257 rows or more also one reached by more rows than the gather's list holds (BW_LIST, read from csrc/), so
    that the remainder carry runs with q aboard.  (One row cannot fill a list: the B = 1 cases.)
"""
import functools
import json
import math
import os
import re

import numpy as np

from golden import cases
from golden import site_cases as sc
from oracle import stdadk_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
ACHIEVED = os.path.join(HERE, "knot_achieved.json")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "st-dadk_amd", "csrc")

ULP = 2.0 ** -24
K_FACTOR = 4.0          # GPU bound = K_FACTOR x the recorded CPU maximum, as optim_cases.py: FMA contraction, the hardware's
                        # division, expf and v_sqrt_f32 -- none of which numpy reproduces
OUTPUTS = ("d_cx", "d_cy", "d_log_bw")
BASES = ("wendland", "gaussian", "triangular")
COMPACT = ("wendland", "triangular")
KINK_BAND = 1e-5
UNREACHED_MARGIN = 1e-4
MIN_UNREACHED = 3
F = np.float32


def f32(x):
    return float(np.float32(x))


@functools.lru_cache(maxsize=None)
def bw_list():
    """BW_LIST of the per-knot gather (compacted candidates per flush), read from the kernels' headers."""
    for name in ("window.h", "l1_bwd_body.h"):
        m = re.search(r"constexpr\s+int\s+BW_LIST\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, name)).read())
        if m:
            return int(m.group(1))
    raise AssertionError("BW_LIST not found under csrc/")


def knot_slabs(B):
    """csrc/knots.hip knot_slabs: ceil(B / 128) in [1, 32]."""
    return min(max(-(-B // 128), 1), 32)


@functools.lru_cache(maxsize=None)
def sup_prime(basis):
    """sup |phi'(r)| over the support, numerically (Wendland 2.50 near r = 0.24, Gaussian exp(-1/2), triangular 1)."""
    r = np.linspace(0.0, 1.0 if basis in COMPACT else 8.0, 800001)
    return float(np.abs(orc.basis_prime(r, basis)).max())


# ------------------------------------------------------------------------------------------------ geometry, scale
def geometry(coords, centers, log_bw, basis):
    """float64 dx, dy, d, r (B, Ks), s (Ks,), reach (B, Ks) bool and the three weights w_j of the bound."""
    x = np.asarray(coords, np.float64).reshape(-1, 2)
    c = np.asarray(centers, np.float64)
    s = np.exp(np.asarray(log_bw, np.float64)) * orc.CALIBRATION_FACTORS[basis]
    dx = x[:, 0:1] - c[None, :, 0]
    dy = x[:, 1:2] - c[None, :, 1]
    d = np.sqrt(dx * dx + dy * dy)
    r = d / s[None, :]
    reach = (r < 1.0) if basis in COMPACT else np.ones(r.shape, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(d > 0, 1.0 / (d * s[None, :]), 0.0)
    return dict(dx=dx, dy=dy, d=d, r=r, s=s, reach=reach, w=(np.abs(dx) * inv, np.abs(dy) * inv, r))


def data_scale(Gabs, geo, basis):
    """S_data (Ks, 3) from |G| (B, Ks) -- or its step-level stand-in."""
    P = sup_prime(basis)
    g = np.where(geo["reach"], np.asarray(Gabs, np.float64), 0.0) * P
    return np.stack([(g * w).sum(0) for w in geo["w"]], axis=1)


def unreached(geo, basis):
    """(Ks,) bool: compact-support knots that no row reaches, with the margin."""
    if basis not in COMPACT:
        return np.zeros(geo["r"].shape[1], bool)
    return geo["r"].min(axis=0, initial=np.inf) > 1.0 + UNREACHED_MARGIN


def near_edge(geo, basis):
    """(B, Ks) bool: pairs inside the kink band of a compact-support basis."""
    if basis not in COMPACT:
        return np.zeros(geo["r"].shape, bool)
    return np.abs(geo["r"] - 1.0) <= KINK_BAND


def redraw(rs, coords, centers, log_bw, basis, fixed, bad_of):
    """Redraw (uniform in the unit square) the rows `bad_of(geo)` flags until none is left; rows < `fixed` are placed
    rows and may not be flagged.  Returns the geometry of the final coordinates."""
    for _ in range(200):
        geo = geometry(coords, centers, log_bw, basis)
        bad = np.nonzero(bad_of(geo))[0]
        if bad.size == 0:
            return geo
        assert bad.min() >= fixed, ("a placed row violates a condition of the inputs", bad[:8])
        coords[bad] = rs.uniform(0.0, 1.0, (bad.size, 2)).astype(F)
    raise AssertionError("rows still violate the conditions after 200 redraws")


# ------------------------------------------------------------------------------------------------ a. embedding level
EMB_SHAPES = [(B, 65) for B in (0, 1, 3, 127, 128, 129, 130, 4096, 4097, 4225)] \
    + [(129, Ks) for Ks in (1, 63, 64, 200)] + [(4225, 200)]
EMB_CASES = [dict(name=f"emb_{basis}_B{B}_K{Ks}", level="emb", basis=basis, B=B, Ks=Ks)
             for basis in BASES for B, Ks in EMB_SHAPES]
# c. the module's own autograd (SpatialBasisEmbedding, learnable): the two-level grid of the round-2 test, perturbed as
# there (centres by N(0, 0.03), log-bandwidths by N(0, 0.2)), above the slab cap; the reach-all / reach-nothing classes on top
MODULE_GRID = [25, 81]
MODULE_CASES = [dict(name=f"module_{basis}_B4225", level="emb", basis=basis, B=4225, Ks=sum(MODULE_GRID), grid=MODULE_GRID)
                for basis in BASES]
EMB_WIDE = (8, 3)       # d_phi = wide[:, 3:3 + Ks] of a (B, Ks + 8) tensor: ld > Ks, base 12 bytes past a 16-byte boundary
S_ALL, S_NONE = 3.0, 1e-3        # support radii that reach every row of the unit square / none but a row on the knot


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31 - 1)


def emb_on_knots(case):
    """Knots the first min(B, 5) rows sit on: the first knots that are not of the reach-nothing class."""
    ks = [k for k in range(case["Ks"]) if k % 8 != 2]
    return ks[:min(case["B"], 5)]


def emb_inputs(case):
    """coords (B, 2), G (B, Ks), centers (Ks, 2), log_bw (Ks,), all float32.  Centres uniform in [-0.1, 1.1]^2; support
    radii: knot k % 8 == 1 reaches every row, k % 8 == 2 none, the rest 0.05 .. 0.6; rows uniform in the unit square,
    the first min(B, 5) exactly on knots.  MODULE_CASES: the perturbed grid and its bandwidths in place of the uniform
    draws."""
    B, Ks, basis = case["B"], case["Ks"], case["basis"]
    rs = np.random.RandomState(_seed(case["name"]))
    if case.get("grid"):
        init, bw, _ = orc.uniform_knots(case["grid"])
        centers = (init + rs.normal(0.0, 0.03, (Ks, 2)).astype(F)).astype(F)
        s = bw.astype(np.float64) * orc.CALIBRATION_FACTORS[basis] * np.exp(rs.normal(0.0, 0.2, Ks))
    else:
        centers = rs.uniform(-0.1, 1.1, (Ks, 2)).astype(F)
        s = rs.uniform(0.05, 0.6, Ks)
    k = np.arange(Ks)
    s = np.where(k % 8 == 1, S_ALL, np.where(k % 8 == 2, S_NONE, s))
    log_bw = np.log(s / orc.CALIBRATION_FACTORS[basis]).astype(F)
    coords = rs.uniform(0.0, 1.0, (B, 2)).astype(F)
    on = emb_on_knots(case)
    coords[:len(on)] = centers[on]
    G = rs.standard_normal((B, Ks)).astype(F)
    if basis in COMPACT:
        none = k % 8 == 2
        redraw(rs, coords, centers, log_bw, basis, len(on),
                lambda geo: near_edge(geo, basis).any(1) | (geo["r"][:, none] <= 1.0 + UNREACHED_MARGIN).any(1))
    return dict(coords=coords, G=G, centers=centers, log_bw=log_bw)


def emb_eval(case, inp):
    """The evaluated case the comparator takes: float64 reference, scale, unreached knots."""
    geo = geometry(inp["coords"], inp["centers"], inp["log_bw"], case["basis"])
    dc, dlb = orc.knot_backward(inp["coords"].reshape(-1, 2), inp["centers"], inp["log_bw"], inp["G"], case["basis"])
    return dict(name=case["name"], basis=case["basis"], ref=np.concatenate([dc, dlb[:, None]], 1),
                S=data_scale(np.abs(inp["G"].astype(np.float64)), geo, case["basis"]),
                unreached=unreached(geo, case["basis"]), geo=geo)


# ------------------------------------------------------------------------------------------------ b. step level
K_TEMPORAL = [10, 15]
# stdadk_knot_train settings; every one runs on every step case.  Between them: damping off / threshold 0 with strength 5 /
# threshold 0.02 with strength 1, domain weight 0 / 0.5, movement weight 0 / 0.1, penalty_grad_scale 1 / 0.5, loss_sum
# given / None.
KT_SETTINGS = {
    "damping_off": dict(damping=False, thr=0.02, strength=1.0, dom_w=0.5, mov_w=0.1, pgs=1.0, loss=True),
    "thr0_s5": dict(damping=True, thr=0.0, strength=5.0, dom_w=0.5, mov_w=0.0, pgs=1.0, loss=True),
    "thr02_s1_half": dict(damping=True, thr=0.02, strength=1.0, dom_w=0.5, mov_w=0.1, pgs=0.5, loss=True),
    "no_weights": dict(damping=True, thr=0.02, strength=1.0, dom_w=0.0, mov_w=0.0, pgs=1.0, loss=True),
    "no_loss": dict(damping=True, thr=0.0, strength=5.0, dom_w=0.0, mov_w=0.1, pgs=0.5, loss=False),
}


def _step_case(route, basis, ks, hidden, p, B, batch="uniform"):
    name = f"{route}_{basis}_h{hidden[0]}_p{p}_B{B}"
    return dict(name=name, level="step", route=route, basis=basis, ks=list(ks), hidden=list(hidden), p=p, B=B,
                batch=batch)


DENSE_CASES = [_step_case("dense", basis, [9, 25], [32, 16], p, B)
               for basis in BASES for p in (0, 3) for B in (1, 257, 4225)]
WINDOW_CASES = [_step_case("window", basis, [25, 81, 121], hidden, p, B, "crowded" if B == 1003 else "uniform")
                for basis in COMPACT for hidden in ([128, 64], [256, 128]) for p in (0, 3) for B in (1, 257, 1003)]
STEP_CASES = DENSE_CASES + WINDOW_CASES
ALL_CASES = EMB_CASES + MODULE_CASES + STEP_CASES
assert len({c["name"] for c in ALL_CASES}) == len(ALL_CASES)


def step_cfg(case):
    return dict(p=case["p"], k_spatial_centers=case["ks"], k_temporal_centers=K_TEMPORAL, hidden_dims=case["hidden"],
                layernorm=True, basis=case["basis"], output_dim=1, B=case["B"], seed=_seed(case["name"]) % 100000,
                learnable=True)


def engineered_knots(ks):
    """Indices into the knot table of the knots the step cases set by hand, all of the finest (last) level, side >= 5:
    k = off + ix * side + iy."""
    n = ks[-1]
    side, off = int(math.isqrt(n)), sum(ks) - n
    a, e = side // 2, side - 1
    at = lambda ix, iy: off + ix * side + iy                                              # noqa: E731
    return dict(corner0=at(0, 0), corner1=at(e, e), x_lo=at(0, a), x_hi=at(e, a), y_lo=at(a, 0), y_hi=at(a, e),
                small_move=at(1, 1), tiny=[at(1, 2), at(1, 3), at(3, 1)], one_row=at(3, 2),
                on=[1, 2, 3, at(2, 2), at(2, 3)])


ONE_ROW_S = 4e-3        # support radius of the knot exactly one row reaches; that row sits at r = 0.56 from it


def step_knots(case):
    """(centers, centers_init, log_bw) float32: the grid knots perturbed as cases.knot_perturbation does, then by hand
    -- two corner knots left where they started (coordinates exactly 0.0 and 1.0, m == 0), four edge knots pushed out
    of the unit square on each side (moved 0.03 .. 0.05), one interior knot moved by 0.005, three knots whose support
    reaches nothing and one that exactly one row reaches."""
    cfg = step_cfg(case)
    init, bw, _ = orc.uniform_knots(case["ks"])
    dc, dlb = cases.knot_perturbation(cfg)
    centers = (init + dc).astype(F)
    log_bw = (np.log(bw.astype(np.float64)).astype(F) + dlb).astype(F)
    e = engineered_knots(case["ks"])
    for k in (e["corner0"], e["corner1"]):
        centers[k] = init[k]
    centers[e["x_lo"]] = init[e["x_lo"]] + F([-0.03, 0.01])
    centers[e["x_hi"]] = init[e["x_hi"]] + F([0.04, -0.01])
    centers[e["y_lo"]] = init[e["y_lo"]] + F([0.01, -0.02])
    centers[e["y_hi"]] = init[e["y_hi"]] + F([-0.02, 0.05])
    centers[e["small_move"]] = init[e["small_move"]] + F([0.003, -0.004])
    cal = orc.CALIBRATION_FACTORS[case["basis"]]
    if case["basis"] in COMPACT:
        log_bw[e["tiny"]] = F(math.log(S_NONE / cal))
        log_bw[e["one_row"]] = F(math.log(ONE_ROW_S / cal))
    return centers.astype(F), init.astype(F), log_bw


def step_inputs(case):
    """dict(cfg, X, coords, t, y, state, centers, centers_init, log_bw, params): everything float32.  Rows uniform in
    the unit square or (batch 'crowded') crowded into one binning cell as site_cases.one_cell has them; with 257 rows
    or more the first five sit exactly on knots and the sixth is the one row of the one-row knot."""
    cfg, B, p, basis = step_cfg(case), case["B"], case["p"], case["basis"]
    rs = np.random.RandomState(cfg["seed"] + 17)
    centers, init, log_bw = step_knots(case)
    e = engineered_knots(case["ks"])
    if case["batch"] == "crowded":
        b = sc.batch(sc.one_cell(), B, cfg["seed"] + 18, p)
        X, coords, t = b["X"], b["coords"].copy(), b["t"]
    else:
        coords = rs.uniform(0.0, 1.0, (B, 2)).astype(F)
        t = (rs.randint(0, sc.T_GRID, size=(B, 1)).astype(F) / F(sc.T_GRID - 1)).astype(F)
        X = rs.standard_normal((B, p)).astype(F)
    fixed = 0
    if B >= 257:
        coords[:5] = centers[e["on"]]
        fixed = 5
        if basis in COMPACT:
            coords[5] = centers[e["one_row"]] + F([0.002, 0.001])
            fixed = 6
    if basis in COMPACT:
        quiet = e["tiny"] + [e["one_row"]]

        def bad_of(geo):
            close = geo["r"][:, quiet] <= 1.0 + UNREACHED_MARGIN
            if fixed == 6:
                close[5, 3] = False                           # the one row of the one-row knot
            return near_edge(geo, basis).any(1) | close.any(1)
        redraw(rs, coords, centers, log_bw, basis, fixed, bad_of)
    y = (sc.smooth_field(coords, t)[:, None] + 0.1 * rs.standard_normal((B, 1))).astype(F)
    state = cases.make_state(cfg)
    params = dict(state)
    params["spatial_basis.centers"] = centers
    params["spatial_basis.log_bandwidths"] = log_bw
    return dict(cfg=cfg, X=X, coords=coords, t=t, y=y, state=state, centers=centers, centers_init=init,
                log_bw=log_bw, params=params)


def step_pass(inp, dtype=np.float64):
    """Forward, MSE and backward of the MLP at `dtype` with the oracle's own functions: (y_pred, dZ0 (B, H0), W0)."""
    cfg = inp["cfg"]
    tc, tb = orc.temporal_knots(cfg["k_temporal_centers"])
    bw = np.exp(inp["log_bw"].astype(dtype))
    phi = orc.spatial_basis(inp["coords"], inp["centers"], bw, cfg["basis"], dtype)
    psi = orc.temporal_basis(inp["t"], tc, tb, dtype)
    feat = orc.features(inp["X"], phi, psi, cfg["p"])
    nh = len(cfg["hidden_dims"])
    yp, cache = orc.mlp_forward(feat, inp["state"], nh, cfg["layernorm"], dtype)
    dy = (2.0 * (yp - inp["y"].astype(dtype)) / yp.size).astype(dtype)
    _, dz0 = orc.mlp_backward(dy, cache, inp["state"], nh, cfg["layernorm"], dtype, return_dz0=True)
    return yp, dz0, np.asarray(inp["state"]["mlp.0.weight"], dtype=dtype)


def step_data(case, inp):
    """The float64 data term of a step case: y, the MSE, the plain knot gradients (oracle.learnable_step_grads without
    penalties or damping), their scale, the unreached knots."""
    cfg, basis = inp["cfg"], case["basis"]
    yp, loss, grads = orc.learnable_step_grads(inp["X"], inp["coords"], inp["t"], inp["y"], inp["params"], cfg, {},
                                               inp["centers_init"])
    _, dz0, W0 = step_pass(inp, np.float64)
    p, Ks = cfg["p"], len(inp["log_bw"])
    geo = geometry(inp["coords"], inp["centers"], inp["log_bw"], basis)
    Gabs = np.abs(dz0) @ np.abs(W0[:, p:p + Ks])
    return dict(name=case["name"], basis=basis, y=yp, loss=loss, dc=grads["spatial_basis.centers"],
                dlb=grads["spatial_basis.log_bandwidths"], S=data_scale(Gabs, geo, basis),
                unreached=unreached(geo, basis), geo=geo, dz0=dz0, W0=W0, centers=inp["centers"],
                centers_init=inp["centers_init"])


def finish64(dc, S, centers, centers_init, kt, mutate=None):
    """What stdadk_knot_backward_f32 adds with a stdadk_knot_train `kt` (a KT_SETTINGS entry; None: nothing), in float64
    on the float32 values the kernel receives: (d_centers, S of the centres, weighted penalty).  `mutate` states a
    wrong finish for tests/test_knot_cases_cpu.py: 'lo_sign', 'damp_first', 'no_pgs'."""
    dc, Sc = np.asarray(dc, np.float64), np.asarray(S, np.float64)[:, :2]
    if kt is None:
        return dc.copy(), Sc.copy(), 0.0
    c, ci = np.asarray(centers, np.float64), np.asarray(centers_init, np.float64)
    dom_w, mov_w, pgs = f32(kt["dom_w"]), f32(kt["mov_w"]), f32(kt["pgs"])
    if mutate == "no_pgs":
        pgs = 1.0
    pen_dom, g_dom = orc.domain_penalty(c)
    pen_mov, g_mov = orc.movement_penalty(c, ci)
    if mutate == "lo_sign":
        g_dom = np.abs(g_dom)
    pen_g = pgs * (dom_w * g_dom + mov_w * g_mov)
    f = orc.damping_factor(c, ci, f32(kt["thr"]), f32(kt["strength"])) if kt["damping"] else np.ones((len(c), 1))
    out = f * dc + pen_g if mutate == "damp_first" else f * (dc + pen_g)
    v = np.maximum(0.0 - c, 0.0) + np.maximum(c - 1.0, 0.0)
    S_out = f * (Sc + pgs * (dom_w * np.abs(2.0 * v) + mov_w * np.abs(2.0 * (c - ci))))
    return out, S_out, dom_w * pen_dom + mov_w * pen_mov


def step_eval(data, kt_name, mutate=None):
    """The evaluated case of step_data's result under one KT_SETTINGS entry (None: the plain data gradient)."""
    kt = KT_SETTINGS[kt_name] if kt_name is not None else None
    dc, Sc, pen = finish64(data["dc"], data["S"], data["centers"], data["centers_init"], kt, mutate)
    return dict(name=f"{data['name']}:{kt_name}", basis=data["basis"], ref=np.concatenate([dc, data["dlb"][:, None]], 1),
                S=np.concatenate([Sc, data["S"][:, 2:]], 1), unreached=data["unreached"], geo=data["geo"], penalty=pen,
                data_S=data["S"], kt=kt)


# ------------------------------------------------------------------------------------------------ conditions
def knot_classes(centers, centers_init, thr):
    """Counts of the knots of every class a knot_train case must hold."""
    c, m = np.asarray(centers, np.float64), np.asarray(centers, np.float64) - np.asarray(centers_init, np.float64)
    dist = np.sqrt((m * m).sum(1))
    return dict(x_below=int((c[:, 0] < 0).sum()), x_above=int((c[:, 0] > 1).sum()), y_below=int((c[:, 1] < 0).sum()),
                y_above=int((c[:, 1] > 1).sum()), exactly0=int((c == 0.0).any(1).sum()),
                exactly1=int((c == 1.0).any(1).sum()), unmoved=int((dist == 0).sum()),
                below_thr=int(((dist > 0) & (dist < thr)).sum()), above_thr=int((dist > thr).sum()))


def reach_classes(geo):
    n = geo["reach"].sum(0)
    return dict(over_list=int((n > bw_list()).sum()), ragged8=int(((n % 8 != 0) & (n > 0)).sum()), one=int((n == 1).sum()))


def check_conditions(case, inp, ev):
    """Every condition of the module docstring for one case (`ev`: emb_eval's or step_data's result)."""
    basis, geo = case["basis"], ev["geo"]
    B, Ks = geo["r"].shape
    for a in (inp["coords"], inp["centers"], inp["log_bw"]):
        assert a.dtype == np.float32
    if basis in COMPACT:
        assert not near_edge(geo, basis).any(), case["name"]
        need = MIN_UNREACHED if Ks >= 24 else 0
        assert ev["unreached"].sum() >= need, (case["name"], int(ev["unreached"].sum()))
        assert np.all(ev["S"][ev["unreached"]] == 0.0)
        assert np.all(geo["reach"].sum(0)[ev["unreached"]] == 0)
    on = emb_on_knots(case) if case["level"] == "emb" else (engineered_knots(case["ks"])["on"] if B >= 257 else [])
    for row, k in enumerate(on):
        assert geo["d"][row, k] == 0.0 and np.array_equal(inp["coords"].reshape(-1, 2)[row], inp["centers"][k])
    if case["level"] == "step":
        for name, kt in KT_SETTINGS.items():
            cl = knot_classes(inp["centers"], inp["centers_init"], f32(kt["thr"]))
            for k, n in cl.items():
                assert n >= 1 or (k == "below_thr" and kt["thr"] == 0.0), (case["name"], name, k)
        if case["route"] == "window":
            rc = reach_classes(geo)
            assert rc["one"] >= 1 and rc["ragged8"] >= 1, (case["name"], rc)
            assert rc["over_list"] >= 1 or B < 257, (case["name"], rc)


# ------------------------------------------------------------------------------------------------ comparator
@functools.lru_cache(maxsize=None)
def bounds():
    """{output: K} of the GPU tests: K_FACTOR x the recorded maximum of the float32 restatement."""
    rec = json.load(open(ACHIEVED))
    return {k: K_FACTOR * float(rec["max"][k]) for k in OUTPUTS}


def normalised(got_dc, got_dlb, ev):
    """{output: (worst |got - ref| / (2^-24 S) over the knots with S > 0, its knot)} -- no assertion."""
    got = np.concatenate([np.asarray(got_dc, np.float64).reshape(-1, 2), np.asarray(got_dlb, np.float64).reshape(-1, 1)], 1)
    err = np.abs(got - ev["ref"])
    out = {}
    for j, name in enumerate(OUTPUTS):
        pos = ev["S"][:, j] > 0
        if not pos.any():
            out[name] = (0.0, -1)
            continue
        u = np.where(pos, err[:, j] / np.where(pos, ULP * ev["S"][:, j], 1.0), 0.0)
        k = int(np.argmax(np.where(np.isfinite(u), u, np.inf)))
        out[name] = (float(u[k]) if np.isfinite(u[k]) else float("inf"), k)
    return out


def compare_knots(got_dc, got_dlb, case, K=None):
    """One result against its evaluated case (emb_eval / step_eval).  Asserts that every output is finite, that every
    output whose scale is 0 -- the data outputs of unreached knots among them -- is exactly 0.0, and the bound
    |got - ref| <= K 2^-24 S per knot and output (K: bounds() unless given).  Returns {output: (worst normalised
    error, knot)} for printing."""
    ev = case
    K = bounds() if K is None else K
    got_dc, got_dlb = np.asarray(got_dc), np.asarray(got_dlb)
    Ks = ev["ref"].shape[0]
    assert got_dc.shape == (Ks, 2) and got_dlb.shape == (Ks,), (ev["name"], got_dc.shape, got_dlb.shape)
    assert np.isfinite(got_dc).all() and np.isfinite(got_dlb).all(), (ev["name"], "not finite")
    got = np.concatenate([got_dc.astype(np.float64), got_dlb.astype(np.float64)[:, None]], 1)
    un = ev["unreached"]
    data_S = ev.get("data_S", ev["S"])
    assert np.all(data_S[un] == 0.0)
    # an unreached knot: exactly zero in the data outputs -- with a knot_train the centres then hold the penalty alone,
    # which the bound below pins (S is the penalty's own magnitude), d_log_bw stays exactly zero
    plain = ev["S"][un] == 0.0
    assert np.all(got[un][plain] == 0.0), (ev["name"], "unreached knots not exactly zero", np.nonzero(un)[0][:8])
    zero = ev["S"] == 0.0
    assert np.all(got[zero] == 0.0), (ev["name"], "nothing is added here, yet not exactly zero",
                                      np.argwhere(zero & (got != 0.0))[:8].tolist())
    worst = normalised(got_dc, got_dlb, ev)
    for name in OUTPUTS:
        assert worst[name][0] <= K[name], (ev["name"], name, "knot", worst[name][1], worst[name][0], "K", K[name])
    return worst


def fmt(worst):
    return ", ".join(f"{k} {worst[k][0]:.2f} (knot {worst[k][1]})" for k in OUTPUTS)
