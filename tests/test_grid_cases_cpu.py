"""The site x time grid cases of tests/golden/grid_cases.py, checked where no GPU is needed: that no library call of
any case sees more than site_cases.MAX_ROWS_PER_CELL rows in one binning cell; that every case reaches the tiles,
chunks and site slices it is named after; that the comparator of tests/test_gpu_predict_grid.py passes an honest
float32 evaluation and fails the four index mistakes a grid pass can make; and, in a child process under
STDADK_DRY_RUN=1 (every entry point validates and plans, nothing is launched, host tensors), that predict_grid and
score_grid of every model return and call the entry points of the model's recorded route.

This file is its own driver, like tests/test_engine_call_trace.py: `python tests/test_grid_cases_cpu.py` with
STDADK_DRY_RUN=1 prints the record as JSON."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from golden import cases                      # noqa: E402
from golden import grid_cases as gc           # noqa: E402
from golden import site_cases as sc           # noqa: E402


# ------------------------------------------------------------------------------------------------ models
def build(name, device):
    """Model `name` of grid_cases.MODELS on `device` in eval mode, parameters from cases.make_state (as
    test_gpu_parity.build_model / build_quantile_model / build_learn_model and test_gpu_round2._scattered_model do);
    `engine`: a TrainStep is constructed on it first, so W0 becomes a .t() view of engine-owned (in,out) storage.
    Returns (model, engine or None): the caller keeps the engine alive."""
    import torch
    from stnf.models import STInterpMLP
    spec = gc.MODELS[name]
    cfg, kind = spec["cfg"], spec["kind"]
    kw = dict(p=0, k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=cfg["k_temporal_centers"],
              hidden_dims=cfg["hidden_dims"], dropout=0.0, layernorm=cfg["layernorm"],
              spatial_basis_function=cfg["basis"], output_dim=cfg["output_dim"])
    if kind == "delta":
        kw["use_delta_reparameterization"] = True
    if kind == "learn":
        kw["spatial_learnable"] = True
    if kind == "scattered":
        s = spec["scattered"]
        rs = np.random.RandomState(s["seed"])
        pts = np.concatenate([rs.uniform(0, 1, (12000, 2)), 0.3 + 0.05 * rs.standard_normal((6000, 2))]).astype(np.float32)
        np.random.seed(s["seed"])
        kw.update(spatial_init_method="random_site", train_coords=pts)
    m = STInterpMLP(**kw)
    st = cases.make_state(cfg)
    named = dict(m.named_parameters())
    with torch.no_grad():
        for k, v in st.items():
            assert tuple(named[k].shape) == v.shape, k
            named[k].copy_(torch.from_numpy(v.copy()))
        sb = m.spatial_basis
        if kind == "learn":
            cen, lbw = gc.learn_knots(cfg)
            sb.centers.copy_(torch.from_numpy(cen))
            sb.log_bandwidths.copy_(torch.from_numpy(lbw))
        if kind == "scattered":
            c = sb.centers
            c[3] = torch.tensor([-0.04, 0.5]); c[7] = torch.tensor([1.03, -0.02]); c[11] = torch.tensor([0.5, 1.06])
            sb._bandwidths[5] *= 2.0; sb._bandwidths[100] *= 1.7
    assert set(st) == {k for k in named if not k.startswith("spatial_basis.")}, sorted(set(st) ^ set(named))
    m.force_window_path = spec["force_window"]
    m = m.to(device)
    eng = None
    if spec["engine"]:
        from stnf.engine import TrainStep
        eng = TrainStep(m, lr=1e-3, max_batch=64)
        w0 = m._body[0].weight
        assert not w0.is_contiguous() and w0.t().is_contiguous()
    return m.eval(), eng


# ------------------------------------------------------------------------------------------------ the dry-run driver
_NAMES = {"stdadk_spatial_partial_f32": ("spatial_partial", 4), "stdadk_temporal_partial_f32": ("temporal_partial", 4),
          "stdadk_forward_parts_f32": ("forward_parts", None), "stdadk_forward_f32": ("forward", 6),
          "stdadk_gemm_f32": ("gemm", 6), "stdadk_rbf_build_f32": ("rbf_build", 3),
          "stdadk_grid_score_f32": ("grid_score", 4)}


def _record():
    """{case: dict(calls [[entry point, rows]], keep_none, shape, score (smallest case of a model only))}: the entry
    points predict_grid called, with the rows of each call (forward_parts: S x n)."""
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    import torch
    from stnf import _native as N
    from stnf.engine import Predictor
    real = N.lib()
    log = []

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in _NAMES:
                return fn

            def call(*args):
                short, pos = _NAMES[name]
                log.append([short, int(args[3]) * int(args[5]) if pos is None else int(args[pos])])
                return fn(*args)
            return call

    proxy = Proxy()
    N.lib = lambda: proxy
    dev = torch.device("cpu")
    out = {}
    for name in gc.MODELS:
        m, eng = build(name, dev)
        small = gc.smallest_case(name)
        for case in (k for k, c in gc.CASES.items() if c["model"] == name):
            c = gc.CASES[case]
            coords, tv = (torch.from_numpy(a) for a in gc.inputs(case))
            pr = Predictor(m, chunk=c["chunk"])
            del log[:]
            y = pr.predict_grid(coords, tv, max_rows=c["max_rows"])
            rec = dict(calls=[list(x) for x in log], keep_none=pr.state.keep is None, shape=list(y.shape))
            if case == small:
                del log[:]
                S, T = len(coords), len(tv)
                try:
                    accs = pr.score_grid(coords, tv, torch.zeros(T, S), torch.zeros(T, S, dtype=torch.uint8),
                                         max_rows=c["max_rows"])
                    rec["score"] = dict(calls=[list(x) for x in log], shapes=[list(a.shape) for a in accs])
                except RuntimeError as e:
                    rec["score"] = dict(calls=[list(x) for x in log], error=str(e))
            out[case] = rec
        del eng
    return out


_RECORD = []


def _recorded():
    if not _RECORD:
        env = dict(os.environ, STDADK_DRY_RUN="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        _RECORD.append(json.loads(r.stdout))
    return _RECORD[0]


# ------------------------------------------------------------------------------------------------ the cases themselves
def test_every_model_has_a_case_and_p_is_zero():
    assert {c["model"] for c in gc.CASES.values()} == set(gc.MODELS)
    assert all(spec["cfg"]["p"] == 0 for spec in gc.MODELS.values())
    assert len(gc.REFUSED) == 6


@pytest.mark.parametrize("case", list(gc.CASES))
def test_no_call_bins_more_than_the_cell_limit(case):
    """Window route: spatial_partial bins the sites of its call.  Materialising route: nothing is binned.  Expanded
    route: predict() bins n copies of every site per chunk of n slices, in pieces of `chunk` rows."""
    c = gc.CASES[case]
    route = gc.MODELS[c["model"]]["route"]
    coords, _ = gc.inputs(case)
    worst = 0
    if route == "window":
        for s0, n in gc.site_chunks(case):
            worst = max(worst, sc.rows_per_cell(coords[s0:s0 + n]))
    elif route == "expanded":
        for _, n in gc.time_chunks(case):
            rows = np.tile(coords, (n, 1))
            for r0 in range(0, len(rows), c["chunk"]):
                worst = max(worst, sc.rows_per_cell(rows[r0:r0 + c["chunk"]]))
        assert len(coords) * c["T"] <= 67 * 7
    assert worst <= sc.MAX_ROWS_PER_CELL, worst
    if len(coords) == 1:
        assert route != "expanded"


def test_cases_reach_what_they_are_named_after():
    th, tc, sch = gc.tile_heights, gc.time_chunks, gc.site_chunks
    # tiles: 32- and 64-row with S prime, a last tile of one row, T == 1 and S == 1 at the first 32-row size
    for case, h in (("w_depth1-1021x8", 32), ("w_tri-1021x8", 32), ("d_D512-1021x8", 32), ("w_k48_q2-1021x16", 64),
                    ("w_depth8_q8-1021x16", 64), ("d_gauss_q2-1021x16", 64), ("d_gauss_q2_engine-1021x8", 32)):
        S = len(gc.inputs(case)[0])
        assert th(case) == [h] and all(S % d for d in range(2, int(math.isqrt(S)) + 1)), case
    for case, rows, h in (("w_k80_k176_noln-859x19", 16321, 64), ("d_D512-859x19", 16321, 64),
                          ("w_narrow_wide_q4-8161x1", 8161, 32), ("w_narrow_wide_q4-1x8161", 8161, 32),
                          ("default227_learn-1x8161", 8161, 32)):
        S = len(gc.inputs(case)[0])
        assert S * gc.CASES[case]["T"] == rows and rows % h == 1 and th(case) == [h], case
    assert gc.tail_rows(8160) == 16 and gc.tail_rows(16320) == 32 and gc.tail_rows(16321, bf16=True) == 32
    # time chunks
    for case in gc.CASES:
        if gc.CASES[case]["T"] == 7 and gc.CASES[case]["max_rows"]:
            assert tc(case) == [(0, 3), (3, 3), (6, 1)], case
    for case in ("w_k80_k176_noln-1021x11", "default227_delta5-1021x11"):
        assert tc(case) == [(0, 8), (8, 3)] and th(case) == [32, 16], case
    # site chunks
    assert len(sch("w_k48_q2-1003x3-chunk64")) == 16 and sch("w_k48_q2-1003x3-chunk64")[-1] == (960, 43)
    assert len(sch("c2_b257-331x3-chunk64")) == 6 and sch("c2_b257-331x3-chunk64")[-1] == (320, 11)
    assert [n for _, n in sch("w_tri-blobs-x7-chunk128")] == [128, 128, 44]
    assert [n for _, n in sch("s_tri-509x7-chunk256")] == [256, 253]
    assert [n for _, n in sch("w_depth1-listed_twice-x5")] == [64, 64, 2]
    # the 64-row grids on 544 knots at most; the C2 tables at about 1 000 rows at most
    for case, c in gc.CASES.items():
        ks = sum(gc.MODELS[c["model"]]["cfg"]["k_spatial_centers"])
        rows = len(gc.inputs(case)[0]) * c["T"]
        assert rows <= 16336
        assert ks <= 544 or rows <= 8168 + 3 * 1021, case
        assert ks < 10000 or rows <= 1000, case


def test_sites_and_times_are_what_they_say():
    tw = gc.listed_twice()
    assert len(np.unique(tw, axis=0)) == len(tw) - 30 and np.array_equal(tw[:30], tw[-30:])
    u = gc.uniform_sites(1021, 1)
    assert u.min() < 0.0 and u.max() > 1.0 and u.min() >= -0.05 and u.max() <= 1.05
    from oracle import stdadk_oracle as orc
    for case, c in gc.CASES.items():
        coords, tv = gc.inputs(case)
        assert coords.dtype == tv.dtype == np.float32 and coords.shape[1] == 2 and tv.shape == (c["T"],)
        knots = orc.temporal_knots(gc.MODELS[c["model"]]["cfg"]["k_temporal_centers"])[0]
        assert np.isin(tv, knots).any()                                    # exactly on a temporal knot
        if c["T"] >= 3:
            assert tv[1] < 0.0 and np.any(np.diff(tv) < 0) and len(np.unique(tv)) < len(tv), case
        if c["T"] >= 5:
            assert tv[2] in knots and tv[3] > 1.0
    assert len(orc.temporal_knots(gc.MODELS["w_kt1"]["cfg"]["k_temporal_centers"])[0]) == 1


# ------------------------------------------------------------------------------------------------ the comparator's teeth
TEETH = "w_tri-blobs-x7-chunk128"       # S = 300, T = 7: site calls (0,128) (128,128) (256,44), time chunks 3, 3, 1


def _teeth_grids():
    coords, tv = gc.inputs(TEETH)
    model = gc.CASES[TEETH]["model"]
    return coords, tv, gc.grid64(model, coords, tv), gc.grid64(model, coords, tv, dtype=np.float32)


def test_comparator_passes_float32_and_fails_index_mistakes():
    """An honest float32 evaluation of the grid passes the bound with room; each of the four mistakes the host loop
    or the tile addressing can make, applied to that float32 grid, fails it."""
    coords, tv, y64, y32 = _teeth_grids()
    T, S, Q = y64.shape
    honest = gc.grid_error(y32, y64)
    print(f"{TEETH}: float32 oracle against float64 {honest:.2e}")
    assert honest <= 0.5 * gc.TOL
    model = gc.CASES[TEETH]["model"]
    mistakes = {}
    # (T, S) written site-major
    mistakes["site-major"] = y32.transpose(1, 0, 2).reshape(T, S, Q)
    # the rows of one 16-row tile take tp of the next time slice (g / S off by one for that tile)
    flat = y32.reshape(T * S, Q).copy()
    r0 = 16 * 7
    flat[r0:r0 + 16] = y32.reshape(T * S, Q)[r0 + S:r0 + S + 16]
    mistakes["tile shifted by a slice"] = flat.reshape(T, S, Q)
    # t0 dropped in the second max_rows chunk: slices 3..5 computed at the times of slices 0..2
    (_, _), (t0, n), _ = gc.time_chunks(TEETH)
    wrong_t = tv.copy()
    wrong_t[t0:t0 + n] = tv[0:n]
    mistakes["t0 dropped"] = gc.grid64(model, coords, wrong_t, dtype=np.float32)
    # the second site call's rows of sp written at s0 = 0 (sites 128..255 keep what they had: here the right rows)
    s0, ns = gc.site_chunks(TEETH)[1]
    moved = y32.copy()
    moved[:, 0:ns] = y32[:, s0:s0 + ns]
    mistakes["sp slice at s0 = 0"] = moved
    for what, y in mistakes.items():
        e = gc.grid_error(y, y64)
        print(f"  {what}: {e:.2e}")
        assert e > 100 * gc.TOL, (what, e)


# ------------------------------------------------------------------------------------------------ dry run
EXPECTED_CALLS = {"window": {"spatial_partial", "temporal_partial", "forward_parts"},
                  "materialising": {"rbf_build", "gemm", "temporal_partial", "forward_parts"},
                  "expanded": {"forward"}}


@pytest.mark.parametrize("case", list(gc.CASES))
def test_dry_run_takes_the_recorded_route(case):
    """predict_grid returns on host tensors under STDADK_DRY_RUN=1 and calls exactly the entry points of the model's
    route, as often and on as many rows as the case's chunks say; score_grid (the smallest case of every model) makes
    the same calls plus one grid_score per chunk of time slices."""
    rec = _recorded()[case]
    c = gc.CASES[case]
    spec = gc.MODELS[c["model"]]
    route = spec["route"]
    S = len(gc.inputs(case)[0])
    assert rec["shape"] == [c["T"], S, spec["cfg"]["output_dim"]]
    calls = rec["calls"]
    assert {n for n, _ in calls} == EXPECTED_CALLS[route], (route, calls)
    rows = lambda what, cc=calls: [r for n, r in cc if n == what]                          # noqa: E731
    chunks = gc.time_chunks(case)
    if route == "expanded":
        assert sum(rows("forward")) == S * c["T"] and max(rows("forward")) <= c["chunk"]
    else:
        assert rows("forward_parts") == [n * S for _, n in chunks]
        assert rows("temporal_partial") == [c["T"]]
    if route == "window":
        assert rows("spatial_partial") == [n for _, n in gc.site_chunks(case)]
    if route == "materialising":
        assert sum(rows("gemm")) == S and rows("gemm") == rows("rbf_build")
        assert rec["keep_none"] == spec["engine"]
    if case == "d_D256-1030x2":
        assert rows("gemm") == [1024, 6]
    if "score" in rec and spec["cfg"]["output_dim"] > 8:
        # the scoring kernel has STDADK_MAX_Q = 8 check-loss slots per split (include/stdadk.h): a nine-output grid is
        # predicted (above) but not scored, and stdadk_grid_score_f32 says so after the first chunk's predictions
        sco = rec["score"]
        assert "grid_score: Q=9 outside 1..8" in sco["error"] and sco["calls"][-1][0] == "grid_score"
        assert [n for n, _ in sco["calls"][:-1]] == ["forward"]
    elif "score" in rec:
        sco = rec["score"]
        assert "error" not in sco, sco["error"]
        assert sco["shapes"] == [[4, 16], [4, S, 3], [4, c["T"], 3]]
        assert [x for x in sco["calls"] if x[0] != "grid_score"] == calls
        assert rows("grid_score", sco["calls"]) == [n for _, n in chunks]
    assert case != gc.smallest_case(c["model"]) or "score" in rec


if __name__ == "__main__":
    json.dump(_record(), sys.stdout)
    sys.exit(0)
