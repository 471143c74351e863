"""Empirical variograms without a GPU: the contract's known answer worked by hand, the restatements of
tests/golden/variogram_cases.py against each other, the product's host path (stnf.utils.variogram) against them --
alone and through grid_scores of a CPU model --, the comparator's teeth, and the constants the cases restate pinned
against the sources."""
import os
import re

import numpy as np
import pytest
import torch

from golden import variogram_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HAND = dict(coords=[[0, 0], [0.25, 0], [0.75, 0]], z=[[1, 2, 4], [2, np.nan, 7]], p=[[1.5, 2, 3], [2, 5, 6]],
            edges2=[0, 0.1, 0.3, 1.0], lags=2)
# rows (N, SZ, SP, SR) per lag and bin, worked by hand:
#  u = 0   (0,1) d2 = .0625 bin 0: dz -1, dp -.5, dr -.5 | (1,2) d2 = .25 bin 1: dz -2, dp -1, dr -1 at t = 0 only (z[1][1]
#          is NaN) | (0,2) d2 = .5625 bin 2: t = 0: dz -3, dp -1.5, dr -1.5; t = 1: dz -5, dp -4, dr -1
#  u = 1   a = (0, i), b = (1, j), j = 1 never counts.  bin 0 (i = j, d2 = 0): (0,0) dz -1, dp -.5, dr -.5; (2,2) dz -3,
#          dp -3, dr 0; and (1,0): dz 0, dp 0, dr 0.  bin 1: (1,2) dz -5, dp -4, dr -1.  bin 2: (0,2) dz -6, dp -4.5,
#          dr -1.5; (2,0) dz 2, dp 1, dr 1
HAND_ROWS = [[(1, 1, 0.25, 0.25), (1, 4, 1, 1), (2, 34, 18.25, 3.25)],
             [(3, 10, 9.25, 0.25), (1, 25, 16, 1), (2, 40, 21.25, 3.25)]]


def _hand(fn):
    h = HAND
    return fn(np.array(h["p"], dtype=np.float32), np.array(h["z"], dtype=np.float32), None,
              np.array(h["coords"], dtype=np.float32), np.array(h["edges2"]), h["lags"])


@pytest.mark.parametrize("which", ["brute", "exact", "numpy", "product"])
def test_known_answer_by_hand(which):
    from stnf.utils import variogram as V
    fn = {"brute": vc.restate_brute, "exact": vc.restate_exact, "numpy": vc.restate_numpy,
          "product": V.variogram_sums_host}[which]
    acc = _hand(fn)
    assert acc.shape == (4, 2, 3, 4)
    assert np.array_equal(acc[0], np.array(HAND_ROWS, dtype=np.float64))
    assert not acc[1:].any()


def _small_cases():
    k = 0
    for S in (1, 2, 3, 17, 33):
        for nT, L in ((1, 1), (2, 2), (5, 3), (3, 5)):
            split_given, pred, first_zero = vc.toggles(k)
            y, z, code, coords = vc.make_case(S, nT, seed=k, ldy=pred[0] if pred else 1, spread=8 if k % 2 else 32)
            yield (None if pred is None else y[:, pred[1]].reshape(nT, S), z, code if split_given else None, coords,
                   vc.edges_on_attained(coords, (1, 5, 64)[k % 3], first_zero), L)
            k += 1


def test_restatements_agree_on_small_cases():
    """brute == exact bit for bit (both are the exact sums); numpy within the bound, equal counts; and the cases hold
    what they are for: NaN, +-inf, an invalid code, duplicated sites, pairs on an edge and beyond the last."""
    seen = set()
    for pred, z, code, coords, e2, L in _small_cases():
        a, b, c = (f(pred, z, code, coords, e2, L) for f in (vc.restate_brute, vc.restate_exact, vc.restate_numpy))
        assert np.array_equal(a, b)
        assert not vc.compare(c, a), vc.compare(c, a)[:3]
        d2 = vc.sq_dist(coords)
        off = ~np.eye(len(coords), dtype=bool)
        seen |= {n for n, v in (("nan", np.isnan(z).any()), ("inf", np.isposinf(z).any()), ("-inf", np.isneginf(z).any()),
                                ("code 7", code is not None and (code == 7).any()), ("duplicates", (d2[off] == 0).any()),
                                ("on an edge", np.isin(d2[off], e2[1:]).any()), ("beyond", (d2 >= e2[-1]).any()),
                                ("no prediction", pred is None), ("no split", code is None), ("edge0 > 0", e2[0] > 0),
                                ("lags > nT", L > z.shape[0])) if v}
    assert seen == {"nan", "inf", "-inf", "code 7", "duplicates", "on an edge", "beyond", "no prediction", "no split",
                    "edge0 > 0", "lags > nT"}


def test_product_host_path_equals_restatement():
    from stnf.utils import variogram as V
    for pred, z, code, coords, e2, L in _small_cases():
        got = V.variogram_sums_host(pred, z, code, coords, e2, L, block=7)
        bad = vc.compare(got, vc.restate_exact(pred, z, code, coords, e2, L))
        assert not bad, bad[:3]


def test_comparator_has_teeth():
    """One term moved to the neighbouring bin, one pair counted twice inside a diagonal tile, one dropped lag."""
    y, z, code, coords = vc.make_case(33, 3, seed=11)
    pred = y[:, 0].reshape(3, 33)
    e2 = vc.edges_on_attained(coords, 5)
    L = 2
    ref = vc.restate_brute(pred, z, code, coords, e2, L)
    assert not vc.compare(ref.copy(), ref)
    cnt = vc._codes(z, code)
    # a counting pair of lag 0 at t = 0 inside the first tile, whose neighbouring bin exists
    pick = next((i, j) for i in range(vc.TILE) for j in range(i + 1, vc.TILE)
                if cnt[0, i] >= 0 and cnt[0, i] == cnt[0, j] and 0 <= vc.bin_of(vc.sq_dist(coords)[i, j], e2) < 4)
    moved = vc.restate_brute(pred, z, code, coords, e2, L,
                             hook=lambda u, t, i, j, b: [b + 1] if (u, t, i, j) == (0, 0) + pick else [b])
    twice = vc.restate_brute(pred, z, code, coords, e2, L,
                             hook=lambda u, t, i, j, b: [b, b] if (u, t, i, j) == (0, 0) + pick else [b])
    dropped = ref.copy()
    dropped[:, 1] = 0
    for wrong in (moved, twice, dropped):
        assert vc.compare(wrong, ref)
    assert ref[:, 1, :, vc.N_].sum() > 0 and twice[..., vc.N_].sum() == ref[..., vc.N_].sum() + 1
    # a sum off by more than the bound is caught although N agrees; within it, it passes
    c, u, b = np.argwhere(ref[..., vc.N_] > 0)[0]
    near, far = ref.copy(), ref.copy()
    near[c, u, b, vc.SZ] *= 1 + 2.0 ** -52
    far[c, u, b, vc.SZ] *= 1 + (ref[c, u, b, vc.N_] + 1) * 2.0 ** -51
    assert not vc.compare(near, ref) and vc.compare(far, ref)


def test_curves_and_sites():
    from stnf.utils import variogram as V
    acc = _hand(vc.restate_exact)
    cur = V.variogram_curves(acc, np.sqrt(HAND["edges2"]), np.arange(2))
    assert cur["count"].dtype == np.int64 and cur["count"][0].tolist() == [[1, 1, 2], [3, 1, 2]]
    assert cur["gamma_z"][0].tolist() == [[0.5, 2.0, 8.5], [10 / 6, 12.5, 10.0]]
    assert cur["gamma_resid"][0, 0].tolist() == [0.125, 0.5, 0.8125] and cur["gamma_pred"][0, 1, 1] == 8.0
    assert np.isnan(cur["gamma_z"][1:]).all() and cur["lags"].tolist() == [0, 1] and len(cur["edges"]) == 4
    state = np.random.get_state()[1].copy()
    assert V.select_sites(4096).tolist() == list(range(4096))
    drawn = V.select_sites(5000)
    assert len(drawn) == 4096 and (np.diff(drawn) > 0).all() and drawn.max() < 5000
    assert np.array_equal(drawn, V.select_sites(5000)) and len(V.select_sites(5000, "all")) == 5000
    assert V.select_sites(10, [3, 1]).tolist() == [3, 1]
    assert np.array_equal(state, np.random.get_state()[1])                 # the global numpy RNG is not touched
    with pytest.raises(ValueError):
        V.select_sites(10, [10])
    e = V.variogram_edges(np.array([[0, 0], [3, 4]], dtype=np.float32), 5)
    assert np.array_equal(e, np.linspace(0, 2.5, 6))
    for bad in (dict(n_bins=0), dict(n_bins=65), dict(max_dist=0.0)):
        with pytest.raises(ValueError):
            V.variogram_edges(np.zeros((2, 2)), **{"n_bins": 5, **bad})


def test_field_variogram_on_the_host():
    from stnf.utils import field_variogram
    coords, z, code = vc.e2e_field()
    out = field_variogram(z, coords, code, n_bins=6, time_lags=3)
    e2 = out["edges"] * out["edges"]
    ref = vc.restate_exact(None, z, code, coords, e2, 3)
    assert np.array_equal(out["count"], ref[..., vc.N_]) and out["count"].sum() > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.allclose(out["gamma_z"], ref[..., vc.SZ] / (2 * ref[..., vc.N_]), rtol=1e-12, atol=0, equal_nan=True)
    assert not np.nan_to_num(out["gamma_pred"]).any() and not np.nan_to_num(out["gamma_resid"]).any()
    assert out["sites"].tolist() == list(range(vc.E2E_S))


def test_grid_scores_of_a_cpu_model():
    """`variogram: true`: the entry is the restatement of the model's own predictions on the chosen sites; without the
    key the dict and the file are what they are without the feature."""
    from stnf.utils import grid_scores, save_grid_scores_npz
    from stnf.utils.predictions import SPLIT_NAMES
    m = vc.e2e_model()
    coords, z, code = vc.e2e_field()
    S, T = vc.E2E_S, vc.E2E_T
    masks = [code == c for c in (1, 2, 3)]
    config = {"regression_type": "multi-quantile", "quantile_levels": [0.1, 0.5, 0.9]}
    plain = grid_scores(m, z, coords, *masks, config=config)
    assert "variogram" not in plain
    sites = np.arange(3, S, 2)
    got = grid_scores(m, z, coords, *masks, config=dict(config, variogram=True, variogram_bins=7,
                                                         variogram_max_dist=0.6, variogram_time_lags=3,
                                                         variogram_sites=sites))
    assert set(got) == set(plain) | {"variogram"}
    np.testing.assert_equal({k: v for k, v in got.items() if k != "variogram"}, plain)
    with torch.no_grad():
        tv = vc.grid_times(T)
        pred = torch.stack([m(torch.zeros(S, 0), torch.from_numpy(coords), torch.full((S, 1), float(tv[i])))
                            for i in range(T)]).numpy()[:, :, 1]
    edges = np.linspace(0, 0.6, 8)
    ref = vc.restate_exact(pred[:, sites], z[:, sites], code[:, sites], coords[sites], edges * edges, 3)
    assert ref[..., vc.N_].sum() > 0 and (ref[:, 2, :, vc.N_].sum(axis=1) > 0).all()
    for c, name in enumerate(SPLIT_NAMES):
        e = got["variogram"][name]
        assert np.array_equal(e["count"], ref[c, :, :, vc.N_]) and e["count"].shape == (3, 7)
        for key, slot in (("gamma_z", vc.SZ), ("gamma_pred", vc.SP), ("gamma_resid", vc.SR)):
            with np.errstate(divide="ignore", invalid="ignore"):
                want = ref[c, :, :, slot] / (2 * ref[c, :, :, vc.N_])
            assert np.array_equal(np.isnan(e[key]), ref[c, :, :, vc.N_] == 0)
            assert np.allclose(e[key], want, rtol=1e-12, atol=0, equal_nan=True), (name, key)
        assert np.array_equal(e["edges"], edges) and e["lags"].tolist() == [0, 1, 2]
    # defaults: 15 bins up to half the bounding box's diagonal, lag 0 only, every site
    dflt = grid_scores(m, z, coords, *masks, config=dict(config, variogram=True))["variogram"]["train"]
    c64 = coords.astype(np.float64)
    assert dflt["count"].shape == (1, 15)
    assert np.array_equal(dflt["edges"], np.linspace(0, 0.5 * np.hypot(*(c64.max(axis=0) - c64.min(axis=0))), 16))


def test_npz_gains_the_variogram_and_nothing_else(tmp_path):
    from stnf.utils import grid_scores, save_grid_scores_npz
    m = vc.e2e_model(output_dim=1)
    coords, z, code = vc.e2e_field()
    masks = [code == c for c in (1, 2, 3)]
    plain = grid_scores(m, z, coords, *masks)
    got = grid_scores(m, z, coords, *masks, config={"variogram": True, "variogram_bins": 4})
    a = np.load(save_grid_scores_npz(tmp_path / "a", plain))
    b = np.load(save_grid_scores_npz(tmp_path / "b", got))
    extra = sorted(set(b.files) - set(a.files))
    assert extra == sorted(f"variogram/{s}/{n}" for s in ("other", "train", "valid", "test")
                           for n in ("count", "gamma_z", "gamma_pred", "gamma_resid", "edges", "lags"))
    assert not set(a.files) - set(b.files) and not any(k.startswith("variogram") for k in a.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k])
    assert np.array_equal(b["variogram/test/count"], got["variogram"]["test"]["count"])


def test_constants_match_the_sources():
    src = open(os.path.join(ROOT, "st-dadk_amd", "csrc", "variogram.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "stdadk.h")).read()
    from stnf import _native as N
    from stnf.utils import variogram as V
    assert int(re.search(r"constexpr int VG_E = (\d+);", src).group(1)) == vc.TILE
    for name, want in (("N", vc.N_), ("SZ", vc.SZ), ("SP", vc.SP), ("SR", vc.SR), ("MAX_BINS", vc.MAX_BINS),
                       ("MAX_LAGS", vc.MAX_LAGS)):
        assert int(re.search(rf"#define STDADK_VG_{name} (\d+)", hdr).group(1)) == want == getattr(N, f"VG_{name}")
    assert (V.VG_N, V.VG_SZ, V.VG_SP, V.VG_SR, V.MAX_BINS, V.MAX_LAGS) == (0, 1, 2, 3, 64, 16)
    assert all(s % vc.TILE in (0, 1, vc.TILE - 1) or s < vc.TILE for s in vc.SIZES)
    listed = re.search(r"for f in ([^;]+); do", open(os.path.join(ROOT, "st-dadk_amd", "csrc", "build.sh")).read())
    assert "variogram" in listed.group(1).split()
