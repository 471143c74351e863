"""The site x time prediction grid (Predictor.predict_grid / score_grid: stdadk_spatial_partial_f32,
stdadk_temporal_partial_f32, stdadk_forward_parts_f32, the rbf_build + GEMM route and the expanded-rows fallback)
against the float64 oracle on the expanded rows, at the cases of tests/golden/grid_cases.py: 32- and 64-row tiles that
straddle time slices, last tiles of one row, S == 1 and T == 1, grids cut by max_rows and sites cut by chunk, heads of
2 / 4 / 5 / 8 / 9 outputs, depth 1 and 8, no LayerNorm, the delta head, the triangular and Gaussian bases, scattered
and learnable knots, engine-owned (in,out) storage, and the widths the tail refuses.  The other grid tests compare the
grid with Predictor.predict of the same library, where a shared error cancels; here nothing does.

Bound: the project's max|y - y64| <= 1e-5 max(1, max|y64|) (test_gpu_mlp_shapes.TOL, site_cases.TOL).  bf16 operands:
against the emulation of test_gpu_bf16 with that module's bound.  Every test prints what it achieved."""
import numpy as np
import pytest
import torch

from golden import cases
from golden import grid_cases as gc
from oracle import stdadk_oracle as orc

import test_gpu_bf16 as BF
import test_gpu_grid_score as GS
import test_gpu_parity as T
from test_grid_cases_cpu import build

pytestmark = pytest.mark.gpu
TOL = gc.TOL

_MODEL, _REF = {}, {}


def _model(name):
    """(model, engine) of grid_cases.MODELS[name] on the device, built once."""
    if name not in _MODEL:
        _MODEL[name] = build(name, T.dev())
    return _MODEL[name][0]


def _reference(case):
    """(coords, tv, float64 (T, S, Q) grid) of a case, computed once and shared."""
    if case not in _REF:
        coords, tv = gc.inputs(case)
        name = gc.CASES[case]["model"]
        _REF[case] = (coords, tv, gc.grid64(name, coords, tv, _model(name)))
    return _REF[case]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(T.dev())


# ------------------------------------------------------------------ a. the grid, every case
@pytest.mark.parametrize("case", list(gc.CASES))
def test_predict_grid_against_float64(case):
    from stnf import _native as N
    from stnf.engine import Predictor
    c = gc.CASES[case]
    spec = gc.MODELS[c["model"]]
    coords, tv, y64 = _reference(case)
    m = _model(c["model"])
    pr = Predictor(m, chunk=c["chunk"])
    st = pr.state
    # the route the case is recorded under is the one this build takes
    parts = bool(st.flags & N.FLAG_W0_T) and N.forward_parts_supported(st.desc)
    window = parts and not m.spatial_basis.learnable and N.step_uses_window(st.basis, st.desc, st.flags)
    assert ("window" if window else "materialising" if parts else "expanded") == spec["route"]
    got = pr.predict_grid(_dev(coords), _dev(tv), max_rows=c["max_rows"])
    assert got.shape == y64.shape
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    err = gc.grid_error(got, y64)
    tiles = gc.tile_heights(case) if parts else "-"
    print(f"{case} [{spec['route']}, tiles {tiles}]: {y64.shape[0]} x {y64.shape[1]} x {y64.shape[2]} grid y max-abs "
          f"{err:.2e} (of max(1, max|y|) = {max(1.0, float(np.abs(y64).max())):.3g})")
    if spec["route"] == "expanded":
        # the same rows through predict(): a failure names the route
        S, Tn = len(coords), len(tv)
        rows = pr.predict(_dev(np.tile(coords, (Tn, 1))), _dev(np.repeat(tv, S))).cpu().numpy()
        e_rows = gc.grid_error(rows.reshape(y64.shape), y64)
        print(f"    predict() on the expanded rows: {e_rows:.2e}")
        assert e_rows <= TOL, e_rows
    assert err <= TOL, err


@pytest.mark.parametrize("name", ["r_c2_q9", "r_227_h40_24"])
def test_driver_helpers_on_refused_widths(name):
    """stnf.utils.predict_all_times and grid_scores go through the same grid pass: on models the tail refuses they
    return the float64 answer too (the median column Q // 2 at t = t_idx / (T - 1)).  grid_scores on the one-output
    model only: the scoring kernel has eight check-loss slots.  With every prediction within delta of the float64
    one, the mean absolute error moves by at most delta and the mean squared error by 2 delta mae + delta^2."""
    from stnf.utils import grid_scores
    from stnf.utils.predictions import predict_all_times
    spec = gc.MODELS[name]
    Q = spec["cfg"]["output_dim"]
    coords, _ = gc.inputs(gc.smallest_case(name))
    S, Tn = len(coords), 5
    tv = (np.arange(Tn, dtype=np.float32) / np.float32(Tn - 1)).astype(np.float32)
    y64 = gc.grid64(name, coords, tv)[:, :, Q // 2]
    m = _model(name)
    got = predict_all_times(m, coords, Tn, max_rows=2 * S)
    assert got.shape == (Tn, S) and got.dtype == np.float64
    err = gc.grid_error(got, y64)
    print(f"{name}: predict_all_times {Tn} x {S} y max-abs {err:.2e}")
    assert err <= TOL, err
    if Q > 1:
        return
    _, z, _ = GS.inputs(S, Tn, 1, 41)
    sc_ = grid_scores(m, z, coords, max_rows=2 * S)["splits"]["all"]
    fin = np.isfinite(z)
    d = (y64 - np.where(fin, z.astype(np.float64), 0.0))[fin]
    mae, mse = float(np.abs(d).mean()), float((d * d).mean())
    delta = TOL * max(1.0, float(np.abs(y64).max()))
    print(f"{name}: grid_scores mse {sc_['mse']!r} vs {mse!r}, mae {sc_['mae']!r} vs {mae!r}, delta {delta:.2e}")
    assert sc_["rows"] == int(fin.sum())
    assert abs(sc_["mae"] - mae) <= delta and abs(sc_["mse"] - mse) <= 2 * delta * mae + delta * delta


# ------------------------------------------------------------------ b. the three entry points on their own
@pytest.mark.parametrize("case", ["w_k80_k176_noln-1021x11", "w_depth8_q8-1021x16"])
def test_partials_and_forward_parts_against_float64(case):
    """sp and tp against the float64 phi W0^T[spatial rows] and psi W0^T[temporal rows] (no bias: raw), each within
    1e-5 max(1, max|.|); then forward_parts fed the float32 roundings of the FLOAT64 sp and tp against the float64
    forward, so that a layer-0 error cannot hide a tail error, or the reverse.  1021 x 11: the first 8 slices in one
    call (32-row tiles); 1021 x 16: 64-row tiles."""
    from stnf import _native as N
    c = gc.CASES[case]
    name = c["model"]
    cfg = gc.MODELS[name]["cfg"]
    coords, tv, y64 = _reference(case)
    if c["max_rows"]:
        tv, y64 = tv[:8], y64[:8]
    S, Tn = len(coords), len(tv)
    m = _model(name)
    d = T.dev()
    st = m._step_state(d, training=False)
    assert N.step_uses_window(st.basis, st.desc, st.flags) and st.flags & N.FLAG_W0_T
    h0, Ks = cfg["hidden_dims"][0], sum(cfg["k_spatial_centers"])
    ws = torch.empty(N.step_workspace_bytes(st.basis, st.desc, S, st.flags) // 4, device=d)
    sp = torch.full((S, h0), float("nan"), device=d)
    tp = torch.full((Tn, h0), float("nan"), device=d)
    N.spatial_partial(st.basis, st.desc, st.params, _dev(coords), sp, ws, st.flags)
    N.temporal_partial(st.basis, st.desc, st.params, _dev(tv), tp, st.flags)
    W0T = gc.params64(name)["mlp.0.weight"].T                                   # (D, h0)
    _, phi, _ = gc.forward64(name, coords, np.zeros(S, np.float32))
    _, _, psi = gc.forward64(name, coords[:1].repeat(Tn, 0), tv)
    sp64, tp64 = phi @ W0T[:Ks], psi @ W0T[Ks:]
    e_sp, e_tp = gc.grid_error(sp.cpu().numpy(), sp64), gc.grid_error(tp.cpu().numpy(), tp64)
    print(f"{case}: sp {e_sp:.2e} (max|sp| {np.abs(sp64).max():.3g}), tp {e_tp:.2e} (max|tp| {np.abs(tp64).max():.3g})")
    assert e_sp <= TOL and e_tp <= TOL, (e_sp, e_tp)
    y = torch.full((Tn * S, cfg["output_dim"]), float("nan"), device=d)
    N.forward_parts(st.desc, st.params, _dev(sp64.astype(np.float32)), _dev(tp64.astype(np.float32)), y)
    e_y = gc.grid_error(y.cpu().numpy().reshape(y64.shape), y64)
    print(f"{case}: forward_parts on the rounded float64 halves, {gc.tail_rows(Tn * S)}-row tiles: y {e_y:.2e}")
    assert e_y <= TOL, e_y


# ------------------------------------------------------------------ c. bf16 operands
def test_bf16_grid_against_emulation():
    """w_k80_k176_noln on 1021 x 8 (32-row tiles, the most the bf16 + dense-0 instantiations carry) against the float64
    emulation of the bf16 operand rounding (test_gpu_bf16.emulate) with that module's bound EMU_Y."""
    from stnf.engine import Predictor
    name = "w_k80_k176_noln"
    cfg = gc.MODELS[name]["cfg"]
    coords = gc.uniform_sites(1021, 900 + 1021)
    tv = gc.times(8, cfg, 777)
    S, Tn = len(coords), len(tv)
    assert gc.tail_rows(S * Tn, bf16=True) == 32
    m, _ = build(name, T.dev())
    m.compute_dtype = "bf16"
    got = Predictor(m, chunk=4096).predict_grid(_dev(coords), _dev(tv)).cpu().numpy()
    rc, rt = np.tile(coords, (Tn, 1)), np.repeat(tv, S).reshape(-1, 1)
    ye = BF.emulate(BF.features64(cfg, m, None, rc, rt), cases.make_state(cfg), cfg, np.zeros((S * Tn, 1)), BF.DW_BF)[0]
    err = gc.grid_error(got, ye.reshape(Tn, S, 1))
    print(f"{name} bf16 1021 x 8 grid vs emulation: y {err:.2e}")
    assert err <= BF.EMU_Y, err


# ------------------------------------------------------------------ d. scores
@pytest.mark.parametrize("case", ["w_tri-blobs-x7-chunk128", "default227_delta5-1021x11"])
def test_score_grid_against_scores_of_the_float64_grid(case):
    """score_grid (uneven chunks of time slices: the time_tail buffer is used) against test_gpu_grid_score.sums64 of
    the FLOAT64 grid.  Counts exact.  With every prediction within delta = TOL max(1, max|y64|) of the float64 one
    (asserted by test a), a sum of n terms moves by at most: |d| and the check losses n delta (|tau|, |1 - tau| <= 1),
    d^2 by 2 delta sum|d| + n delta^2; plus the 1e-12 relative of test_gpu_grid_score.close for the order of
    summation."""
    from stnf.engine import Predictor
    c = gc.CASES[case]
    coords, tv, y64 = _reference(case)
    Tn, S, Q = y64.shape
    assert len({n for _, n in gc.time_chunks(case)}) == 2
    _, z, code = GS.inputs(S, Tn, Q, 31)
    taus = GS.TAUS[:Q] if Q > 1 else None
    pr = Predictor(_model(c["model"]), chunk=c["chunk"])
    got = [a.cpu().numpy() for a in pr.score_grid(_dev(coords), _dev(tv), _dev(z), _dev(code), quantile_levels=taus,
                                                  max_rows=c["max_rows"])]
    ref = GS.sums64(y64.reshape(Tn * S, Q), z, code, Q // 2, taus, -1, -1)
    delta = TOL * max(1.0, float(np.abs(y64).max()))
    worst = 0.0
    for g, r, what in zip(got[1:], ref[1:], ("site", "time")):                 # (4, ., 3): sum d^2, sum |d|, n
        assert np.array_equal(g[..., 2], r[..., 2]), what
        n = r[..., 2]
        b_abs = n * delta + 1e-12 * np.abs(r[..., 1])
        b_sq = 2 * delta * r[..., 1] + n * delta * delta + 1e-12 * np.abs(r[..., 0])
        assert np.all(np.abs(g[..., 1] - r[..., 1]) <= b_abs) and np.all(np.abs(g[..., 0] - r[..., 0]) <= b_sq), what
        worst = max(worst, float((np.abs(g[..., 1] - r[..., 1]) / np.maximum(b_abs, 1e-300)).max()),
                    float((np.abs(g[..., 0] - r[..., 0]) / np.maximum(b_sq, 1e-300)).max()))
    gs, rs = got[0], ref[0]
    assert np.array_equal(gs[:, [0, 3, 4]], rs[:, [0, 3, 4]]) and gs[:, 0].sum() == np.isfinite(z).sum()
    n = rs[:, 0]
    assert np.all(np.abs(gs[:, 2] - rs[:, 2]) <= n * delta + 1e-12 * np.abs(rs[:, 2]))
    assert np.all(np.abs(gs[:, 1] - rs[:, 1]) <= 2 * delta * rs[:, 2] + n * delta * delta + 1e-12 * np.abs(rs[:, 1]))
    for q in range(Q):
        assert np.all(np.abs(gs[:, 5 + q] - rs[:, 5 + q]) <= n * delta + 1e-12 * np.abs(rs[:, 5 + q])), q
    assert np.all(gs[:, 5 + Q:] == 0)
    print(f"{case}: score_grid vs scores of the float64 grid: counts exact, site / time sums at most {worst:.2e} of "
          f"their bound (delta = {delta:.2e})")
