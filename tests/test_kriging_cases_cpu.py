"""Local ordinary kriging, the half that runs anywhere: the generated cases of tests/golden/kriging_cases.py cover the
edges they must; kriging_weights_host against the long-double bordered solve within c(n) kappa 2^-52 per row (the
reasoning is the generator's head comment), weights summing to 1, the collapsed groups against the uncollapsed system,
kriging_apply_host against long-double sums, the comparator's teeth; fit_variogram on exact model curves and on what it
must refuse; the header and the library; grid_baselines with `baseline_kriging` on the host."""
import json
import os
import re

import numpy as np
import pytest

from golden import kriging_cases as kc
from stnf.utils import baselines as BL
from stnf.utils import kriging as KR
from stnf.utils import variogram as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = np.longdouble


def host_weights(case, tab):
    return KR.kriging_weights_host(tab[0], tab[1], case["k"], case["coords"], case["model"], case["nugget"], case["psill"],
                                   case["range"])


@pytest.fixture(scope="module")
def solved():
    """(case, table, host (w, var), long-double reference) of every generated case: computed once, never changed."""
    out = []
    for case in kc.all_cases():
        tab = kc.table(case)
        out.append((case, tab, host_weights(case, tab), kc.reference(case, tab)))
    return out


def test_the_header_declares_the_entries_and_the_library_exports_them():
    from stnf import _native as N
    hdr = open(os.path.join(ROOT, "include", "stdadk.h")).read()
    assert re.search(r"#define STDADK_ABI_VERSION (\d+)", hdr).group(1) == "10"
    for name, want in (("EXPONENTIAL", 0), ("SPHERICAL", 1), ("GAUSSIAN", 2), ("MAX_COLS", KR.MAX_COLS)):
        assert int(re.search(rf"#define STDADK_KRIGE_{name} (\d+)", hdr).group(1)) == want == getattr(N, f"KRIGE_{name}")
    assert KR.MODELS == kc.MODELS == V.VARIOGRAM_MODELS and KR.MAX_K == kc.MAX_K == BL.MAX_K
    new = {"stdadk_krige_weights_f64", "stdadk_krige_apply_f32"}
    assert new <= set(re.findall(r"\b(stdadk_[a-z0-9_]+)\s*\(", hdr)) and new <= set(N.exported_symbols())
    assert new <= N._OWN_UNIT
    assert "krige" in open(os.path.join(ROOT, "st-dadk_amd", "csrc", "build.sh")).read().split()
    import ctypes
    handle = ctypes.CDLL(N.LIB_PATH)
    assert all(hasattr(handle, name) for name in new)
    src = open(os.path.join(ROOT, "st-dadk_amd", "csrc", "krige.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src


def test_cases_cover_what_they_must(solved):
    cases = [s[0] for s in solved]
    assert {len(c["q"]) for c in cases} >= set(kc.SIZES_M) and {c["k"] for c in cases} >= set(kc.SIZES_K)
    assert all(c["k_tab"] > c["k"] or c["k"] == kc.MAX_K for c in cases) and any(c["k_tab"] > c["k"] for c in cases)
    assert {c["model"] for c in cases} == set(kc.MODELS)
    assert {1 if c["src"] is None else len(c["src"]) for c in cases} == {1, 3}
    for model in kc.MODELS:
        assert {c["nugget"] > 0 for c in cases if c["model"] == model} >= ({True, False} if model != "gaussian" else {True})
    entries = set()                                                     # counting entries of a row, against its k
    groups_apart, on_source, diagonal = set(), False, False
    for case, tab, _, ref in solved:
        S = len(case["coords"])
        counting = ((tab[0][:, :, :case["k"]] >= 0) & (tab[0][:, :, :case["k"]] < S)).sum(axis=2)
        entries |= {(int(n), case["k"]) for n in np.unique(counting)}
        on_source |= bool((tab[1][:, :, 0] == 0.0).any()) and case["nugget"] > 0
        idx = tab[0][:, :, :case["k"]].reshape(-1, case["k"]).astype(np.int64)
        counts, _, rep, members = KR.row_groups(idx, case["coords"].astype(np.float64))
        for r in range(len(idx)):
            for e in np.nonzero(counts[r] & (rep[r] != np.arange(case["k"])))[0]:
                between = [x for x in range(rep[r, e] + 1, e) if counts[r, x] and rep[r, x] != rep[r, e]]
                if between:
                    groups_apart.add(int(members[r, rep[r, e]]))
        if case["range"] < 1e-3:                                        # below the nearest distance: K is diagonal
            near = tab[1][:, :, 0][tab[1][:, :, 0] > 0]
            diagonal |= bool(case["range"] < np.sqrt(near.min()))
    assert {n for n, k in entries} >= {0, 1, 2} and any(n == k - 1 and k > 3 for n, k in entries)
    assert {2, 3} <= groups_apart, groups_apart                        # coincident groups of 2 and 3, not adjacent
    assert on_source and diagonal
    kappas = [s[3][2] for s in solved if s[0]["range"] >= 50.0 and s[0]["model"] != "gaussian"]
    assert kappas and max(k[np.isfinite(k)].max() for k in kappas) > 1e4      # the ill-conditioned range
    # the singular case: every row NaN on the host, exactly singular in long double
    case, tab, (w, var), ref = next(s for s in solved if s[0]["model"] == "gaussian" and s[0]["nugget"] == 0 and s[0]["range"] > 1e6)
    assert np.isnan(w).all() and np.isnan(var).all() and np.isinf(ref[2]).all()


def test_bounded_cases_are_conditioned_as_the_device_comparison_needs(solved):
    achieved = json.load(open(os.path.join(ROOT, "tests", "golden", "kriging_achieved.json")))
    assert achieved["kappa_max"] == kc.KAPPA_MAX and achieved["K_exp"] == achieved["margin"] * max(
        achieved["worst_ratio_w"], achieved["worst_ratio_var"]) and achieved["margin"] == 8.0
    n = len(kc.bitwise_cases())
    for case, _, (w, var), ref in solved[n:]:
        assert case["model"] in ("exponential", "gaussian")
        assert (ref[2] <= kc.KAPPA_MAX).all(), (case["model"], case["k"], ref[2].max())
        assert not np.isnan(w).any() and np.array_equal(np.isnan(var), ref[3] == 0)      # no singular row among them
    assert all(s[0]["model"] == "spherical" or np.isnan(s[2][1]).all() for s in solved[:n])


def test_host_weights_against_the_long_double_solve(solved):
    worst, rows = 0.0, 0
    for case, tab, (w, var), ref in solved:
        ok, ratio = kc.close_to_reference(case, w, var, ref)
        assert ok, (case["model"], len(case["q"]), case["k"], ratio)
        worst, rows = max(worst, ratio), rows + var.size
        some = (ref[3] > 0) & ~np.isnan(var)
        bw = kc.weight_bounds(case, ref)[0]
        assert (np.abs(w.sum(axis=2) - 1.0)[some] <= (case["k"] * bw + case["k"] * 2.0 ** -52)[some]).all()
        assert (w[~some & (ref[3] == 0)] == 0).all()
        S = len(case["coords"])
        assert (w[~((tab[0][:, :, :case["k"]] >= 0) & (tab[0][:, :, :case["k"]] < S)) & ~np.isnan(w)] == 0).all()
    print(f"{rows} rows, worst error / bound {worst:.3g}")
    assert rows > 2000


def test_the_comparator_has_teeth(solved):
    case, tab, (w, var), ref = next(s for s in solved if s[0]["k"] == 8 and s[0]["nugget"] > 0 and len(s[0]["q"]) > 60)
    bw, bv = kc.weight_bounds(case, ref)
    assert kc.close_to_reference(case, w, var, ref)[0]
    moved = w.copy()
    moved[0, 7, 3] += 4.0 * bw[0, 7]
    assert not kc.close_to_reference(case, moved, var, ref)[0]
    moved_var = var.copy()
    moved_var[0, 9] += 4.0 * bv[0, 9]
    assert not kc.close_to_reference(case, w, moved_var, ref)[0]
    gone = w.copy()
    gone[0, 11] = np.nan                           # a regular row reported singular
    assert not kc.close_to_reference(case, gone, var, ref)[0]


def test_collapsed_groups_predict_what_the_uncollapsed_system_predicts(solved):
    checked = 0
    for case, tab, (w, var), ref in solved:
        if case["nugget"] == 0 or case["coords"].shape[0] > 40 and case is not solved[0][0]:
            continue
        idx = tab[0][:, :, :case["k"]].reshape(-1, case["k"]).astype(np.int64)
        counts, _, rep, _ = KR.row_groups(idx, case["coords"].astype(np.float64))
        if not (counts & (rep != np.arange(case["k"]))).any():
            continue
        full = kc.reference(case, tab, collapse=False)
        ok, _ = kc.close_to_reference(case, w, var, full)
        assert ok, (case["model"], case["k"])
        checked += 1
    assert checked >= 3


def test_apply_host_against_long_double_sums(solved):
    values = 0
    for case, tab, (w, var), _ in solved[::3]:
        for zq in ([0.0], [-1.2815515655446004, 0.0, 0.6744897501960817, 1.6448536269514722]):
            out = KR.kriging_apply_host(tab[0], w, var, case["k"], case["z"], zq)
            want, scale = kc.apply_reference(case, tab[0], w, var, zq)
            assert out.dtype == np.float32 and out.shape == want.shape
            assert np.array_equal(np.isnan(out), np.isnan(want))
            fin = ~np.isnan(want)
            # k products and k sums, the product with zq and the last sum in double, then half an ulp of float32
            tol = (2.0 ** -24 * np.abs(want) + (2 * case["k"] + 3) * 2.0 ** -52 * scale[:, :, None])[fin]
            assert (np.abs(out.astype(L) - want)[fin] <= tol).all(), (case["model"], case["k"])
            values += int(fin.sum())
    assert values > 3000
    case, tab, (w, var), _ = solved[2]
    assert np.isnan(KR.kriging_apply_host(tab[0], w, np.full_like(var, np.nan), case["k"], case["z"], [0.0, 1.0])).all()
    neg = KR.kriging_apply_host(tab[0], w, np.full_like(var, -1.0), case["k"], case["z"], [0.0, 1.0])      # var < 0: sd = 0
    assert np.array_equal(neg[:, :, 0], neg[:, :, 1])
    for bad in (dict(k=case["k_tab"] + 1), dict(zq=[0.0] * 9), dict(zq=[np.inf]), dict(z=case["z"][0])):
        a = dict(dict(k=case["k"], zq=[0.0], z=case["z"]), **bad)
        with pytest.raises(ValueError):
            KR.kriging_apply_host(tab[0], w, var, a["k"], a["z"], a["zq"])
    for bad in (dict(model="matern"), dict(nugget=-1.0), dict(nugget=0.0, psill=0.0), dict(range=0.0), dict(psill=np.inf),
                dict(k=0)):
        a = dict(dict(k=case["k"], model="spherical", nugget=0.1, psill=1.0, range=0.5), **bad)
        with pytest.raises(ValueError):
            KR.kriging_weights_host(tab[0], tab[1], a["k"], case["coords"], a["model"], a["nugget"], a["psill"], a["range"])


@pytest.mark.parametrize("model", kc.MODELS)
def test_fit_variogram_recovers_exact_model_curves(model):
    edges = np.linspace(0.0, 0.7, 16)
    mid = 0.5 * (edges[:-1] + edges[1:])
    n = np.arange(15, 0, -1) * 100
    ladder = np.geomspace(0.25 * mid[0], 2.0 * edges[-1], 64)           # the default ladder
    for nugget, psill in ((0.0, 1.5), (0.3, 0.9)):
        on = float(ladder[40])                                           # a range ON the ladder: recovered exactly
        fit = V.fit_variogram(nugget + psill * V.variogram_structure(model, mid, on), n, edges, model)
        assert fit["model"] == model and fit["range"] == on and fit["bins_used"] == 15
        # (the closed form's own rounding: a 2 x 2 solve of sums of 15 terms)
        assert abs(fit["nugget"] - nugget) <= 1e-9 and abs(fit["psill"] - psill) <= 1e-9 and fit["wss"] <= 1e-18
        off = float(np.sqrt(ladder[30] * ladder[31]))                    # between two steps: to the ladder's spacing
        fit = V.fit_variogram(nugget + psill * V.variogram_structure(model, mid, off), n, edges, model)
        assert fit["range"] in (ladder[30], ladder[31])
        step = ladder[31] / ladder[30] - 1.0
        # a range off by the factor (1 + step)^(1/2) moves the curve, and with it nugget and sill, by no more than step
        assert abs(fit["nugget"] - nugget) <= step * (nugget + psill) and abs(fit["psill"] - psill) <= step * (nugget + psill)
    gamma = 0.2 + V.variogram_structure(model, mid, 0.2)
    skipped = V.fit_variogram(np.where(np.arange(15) == 4, np.nan, gamma), np.where(np.arange(15) == 7, 0, n), edges,
                              model, ranges=[0.1, 0.2, 0.4])
    assert skipped["bins_used"] == 13 and skipped["range"] == 0.2 and abs(skipped["nugget"] - 0.2) <= 1e-9


def test_fit_variogram_boundaries_ties_and_refusals():
    edges = np.linspace(0.0, 1.0, 6)
    n = np.full(5, 10)
    flat = V.fit_variogram(np.full(5, 0.7), n, edges)                    # a pure nugget: psill 0, the smallest range wins
    assert flat["psill"] == 0.0 and abs(flat["nugget"] - 0.7) <= 1e-12
    assert flat["range"] == np.geomspace(0.25 * 0.1, 2.0, 64)[0] or flat["wss"] <= 1e-20
    tie = V.fit_variogram(np.full(5, 0.7), n, edges, "spherical", ranges=[0.05, 0.01, 0.02])      # every range fits: the smallest
    assert tie["range"] == 0.01 and abs(tie["nugget"] + tie["psill"] - 0.7) <= 1e-12
    down = V.fit_variogram(np.linspace(1.0, 0.2, 5), n, edges)           # a falling curve: the slope is clamped at 0
    assert down["psill"] == 0.0 and down["nugget"] > 0
    for bad in (dict(gamma=np.zeros(5)), dict(n=np.asarray([5, 5, 0, 0, 0])), dict(gamma=np.asarray([1, np.nan, np.inf, 2, np.nan])),
                dict(model="matern"), dict(edges=edges[:-1]), dict(ranges=[0.0, 1.0]), dict(ranges=[])):
        a = dict(dict(gamma=np.linspace(0.1, 1, 5), n=n, edges=edges, model="exponential", ranges=None), **bad)
        with pytest.raises(ValueError):
            V.fit_variogram(a["gamma"], a["n"], a["edges"], a["model"], a["ranges"])


def _field(T_=6, S=90, seed=8, site_wise=True):
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = (np.sin(5 * coords[:, 0])[None, :] + np.cos(3 * coords[:, 1])[None, :] + rs.standard_normal((T_, S)) * 0.2).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.05] = np.nan
    code = np.broadcast_to(rs.randint(1, 4, size=S), (T_, S)) if site_wise else rs.randint(0, 4, size=(T_, S))
    if site_wise:
        z[:, code[0] == 1] = np.where(np.isnan(z[:, code[0] == 1]), 0.5, z[:, code[0] == 1])
    return coords, z, [code == c for c in (1, 2, 3)]


def test_grid_baselines_without_the_key_is_todays_dict_and_with_it_gains_one_entry():
    coords, z, masks = _field()
    plain = BL.grid_baselines(z, coords, *masks)
    assert set(plain) == {"nearest", "idw", "k", "power", "shared_table", "train_dist"}
    config = {"baseline_kriging": True, "kriging_k": 12, "kriging_levels": [0.05, 0.95]}
    got = BL.grid_baselines(z, coords, *masks, config=config)
    assert set(got) == set(plain) | {"kriging"}
    np.testing.assert_equal({k: v for k, v in got.items() if k != "kriging"}, plain)      # a wider table: the same prefix
    e = got["kriging"]
    assert set(e) >= set(plain["idw"]) | {"variogram_fit", "n_singular", "mean_var", "msse", "model", "k", "levels"}
    assert e["model"] == "exponential" and e["k"] == 12 and e["n_singular"] == 0
    assert set(e["variogram_fit"]) == {"model", "nugget", "psill", "range", "wss", "bins_used"}
    assert e["site_mse"].shape == plain["idw"]["site_mse"].shape and e["time_mse"].shape == plain["idw"]["time_mse"].shape
    assert list(e["levels"]) == [0.05, 0.5, 0.95]
    for s in ("all", "train", "valid", "test"):
        m = e["splits"][s]
        assert m["rows"] == plain["idw"]["splits"][s]["rows"] and np.isfinite([m["mse"], m["crps"], m["coverage"]]).all()
        assert m["reliability"].shape == (3,) and (np.diff(m["reliability"]) >= 0).all() and 0.5 < m["coverage"] <= 1.0
        assert e["mean_var"][s] > 0 and 0.2 < e["msse"][s] < 5.0
    # on a smooth field with noise kriging with a fitted variogram beats copying the nearest site
    assert e["splits"]["test"]["mse"] < plain["nearest"]["splits"]["test"]["mse"]
    with pytest.raises(ValueError):
        BL.grid_baselines(z, coords, *masks, config=dict(config, kriging_levels=[0.9, 0.1]))
    with pytest.raises(ValueError):
        BL.grid_baselines(z, coords, *masks, config=dict(config, kriging_model="matern"))
    with pytest.raises(ValueError):
        BL.grid_baselines(z, coords, *masks, config=dict(config, kriging_k=17))


def test_shared_and_per_time_routes_agree_on_the_host():
    coords, z, masks = _field()
    config = {"baseline_kriging": True, "kriging_model": "spherical", "kriging_params": (0.05, 1.0, 0.6),
              "kriging_levels": [0.1, 0.9]}
    shared = BL.grid_baselines(z, coords, *masks, config=config)
    per_time = BL.grid_baselines(z, coords, *masks, config=dict(config, baseline_per_time=True), max_rows=2 * 90)
    assert shared["shared_table"] and not per_time["shared_table"]
    a, b = shared["kriging"], per_time["kriging"]
    assert a["variogram_fit"]["bins_used"] == 0 and (a["nugget"], a["psill"], a["range"]) == (0.05, 1.0, 0.6)
    # the same tables row for row, the same weights, the same float32 predictions: the sums differ by their chunks only
    for s in a["splits"]:
        for name, v in a["splits"][s].items():
            assert np.allclose(b["splits"][s][name], v, rtol=1e-12, atol=0, equal_nan=True), (s, name)
        assert np.isclose(b["msse"][s], a["msse"][s], rtol=1e-12, equal_nan=True)
        assert np.isclose(b["mean_var"][s], a["mean_var"][s], rtol=1e-12, equal_nan=True)
    assert np.allclose(a["site_mse"], b["site_mse"], rtol=1e-12, equal_nan=True)
    assert np.array_equal(a["time_mse"], b["time_mse"], equal_nan=True)


def test_two_sources_and_no_nugget_follow_from_symmetry():
    """Sources at (0, 0) and (1, 0) with values 1 and 3, every other site a target.  On the perpendicular bisector the
    weights are 1/2 each by symmetry, whatever the model; ON a source, with nugget 0, the prediction is its value and
    the variance 0 -- each to the few roundings of a 2 x 2 solve (kappa < 3 at this range, entries of size 2: 1e-14 is
    fifty of them), which the float32 prediction no longer sees."""
    coords = np.asarray([[0, 0], [1, 0], [.5, .25], [.5, -2], [0, 0], [1, 0]], dtype=np.float32)
    z = np.asarray([[1, 3, 7, 7, 7, 7]], dtype=np.float32)
    train = np.asarray([[1, 1, 0, 0, 0, 0]], dtype=bool)
    for model in kc.MODELS:
        config = {"baseline_kriging": True, "baseline_k": 2, "kriging_model": model, "kriging_params": (0.0, 2.0, 0.8)}
        tab = BL.knn_host(coords, coords, train.astype(np.uint8), 2, True)
        w, var = KR.kriging_weights_host(tab[0], tab[1], 2, coords, model, 0.0, 2.0, 0.8)
        near = lambda a, b: bool(np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-14)      # noqa: E731
        assert near(w[0, 2], [0.5, 0.5]) and near(w[0, 3], [0.5, 0.5]) and var[0, 2] > 0.1
        assert near(w[0, 4], [1.0, 0.0]) and near(var[0, 4], 0.0) and near(w[0, 5], [1.0, 0.0])
        pred = KR.kriging_apply_host(tab[0], w, var, 2, z, [0.0])[0, :, 0]
        assert list(pred[2:]) == [2.0, 2.0, 1.0, 3.0]
        got = BL.grid_baselines(z, coords, train, None, ~train, config=config)
        # test entries: (2 - 7)^2 twice, (1 - 7)^2 and (3 - 7)^2
        assert got["kriging"]["splits"]["test"]["mse"] == (25 + 25 + 36 + 16) / 4
        assert got["kriging"]["n_singular"] == 0


def test_skill_has_the_third_name_only_with_the_entry():
    coords, z, masks = _field()
    model_scores = {"splits": {s: {"mse": 0.1} for s in ("all", "train", "valid", "test", "other")},
                    "site_mse_by_split": np.full((4, 90), 0.1)}
    plain = BL.grid_baselines(z, coords, *masks)
    sk = BL.skill_scores(model_scores, plain)
    assert set(sk["skill"]) == {"nearest", "idw"} and sk["site_skill"].shape == (2, 90)
    got = BL.grid_baselines(z, coords, *masks, config={"baseline_kriging": True})
    sk = BL.skill_scores(model_scores, got)
    assert list(sk["skill"]) == ["nearest", "idw", "kriging"] and sk["site_skill"].shape == (3, 90)
    assert sk["skill"]["kriging"]["test"] == 1.0 - 0.1 / got["kriging"]["splits"]["test"]["mse"]
