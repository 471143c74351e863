"""Neighbour tables and baselines, the half that runs anywhere: knn_host against the independent python restatement on
every generated case of tests/golden/knn_cases.py (indices equal, d2 bit-equal), the comparator's teeth, knn_apply_host
at every power against long-double sums, rasterize_nearest against scipy's griddata(method="nearest") and knn_host
against cKDTree.query with no node left out, grid_baselines on the host (shared and per-time route, a constant field, a
hand-checkable case) and grid_scores' `baseline` entry on a `device: cpu` model."""
import os
import re

import numpy as np
import pytest
import torch

from golden import knn_cases as kc
from stnf.utils import baselines as BL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_table(case):
    return BL.knn_host(case["q"], case["coords"], case["src"], case["k"], case["exclude_self"])


@pytest.fixture(scope="module")
def tables():
    """(case, knn_host's table) of every generated case: computed once, never changed."""
    return [(c, host_table(c)) for c in kc.all_cases()]


def test_constants_are_the_kernels_and_the_header_declares_the_entries():
    from stnf import _native as N
    src = open(os.path.join(ROOT, "st-dadk_amd", "csrc", "knn.hip")).read()
    val = {"kWave": 64}
    for name, expr in re.findall(r"constexpr int (KN_\w+) = ([\w\s*/+-]+);", src):
        if not expr.startswith("0x"):
            val[name] = int(eval(expr, {}, val))
    for name, want in (("KN_Q", kc.WAVES), ("KN_MT", kc.TILE_M), ("KN_SC", kc.CHUNK_S), ("KN_SQ", kc.QUARTER_S),
                       ("KN_FILL", kc.FILL), ("KN_MAX_SPANS", kc.MAX_SPANS)):
        assert val[name] == want, name
    hdr = open(os.path.join(ROOT, "include", "stdadk.h")).read()
    assert re.search(r"#define STDADK_KNN_MAX_K (\d+)", hdr).group(1) == str(kc.MAX_K) == str(BL.MAX_K) == str(N.KNN_MAX_K)
    assert re.search(r"#define STDADK_ABI_VERSION (\d+)", hdr).group(1) == "10"
    new = {"stdadk_knn_workspace_bytes", "stdadk_knn_f32", "stdadk_knn_apply_f32"}
    assert new <= set(re.findall(r"\b(stdadk_[a-z0-9_]+)\s*\(", hdr)) and new <= set(N.exported_symbols())
    assert "knn" in open(os.path.join(ROOT, "st-dadk_amd", "csrc", "build.sh")).read().split()
    # the span rule: one tile of one slice is cut from CHUNK_S + 1 sources on; enough groups are never cut
    assert kc.spans(64, 256, 1) == (1, 256) and kc.spans(64, 257, 1) == (2, 256) and kc.spans(64, 1025, 1) == (5, 256)
    assert kc.spans(64 * 1024, 10 ** 6, 1)[0] == 1 and kc.spans(64, 10 ** 6, 1)[0] == kc.MAX_SPANS
    assert kc.spans(10000, 10000, 1) == (7, 6 * 256) and kc.spans(0, 300, 1)[0] == kc.spans(5, 0, 1)[0] == 0


def test_cases_cover_what_they_must():
    cases = kc.all_cases()
    assert {len(c["q"]) for c in cases} >= set(kc.SIZES_M) and {len(c["coords"]) for c in cases} >= set(kc.SIZES_S)
    assert {c["k"] for c in cases} == set(kc.SIZES_K)
    assert {1 if c["src"] is None else len(c["src"]) for c in cases} == set(kc.SLICES)
    assert any(c["src"] is None for c in cases) and any(c["exclude_self"] for c in cases)
    assert any(c["src"] is not None and 0 < (c["src"][0] != 0).sum() < c["k"] for c in cases)      # fewer than k sources
    assert any(c["src"] is not None and not c["src"][-1].any() for c in cases)                     # none in a slice
    assert any(np.isnan(c["coords"]).any() and np.isnan(c["q"]).any() for c in cases)
    assert any(kc.spans(len(c["q"]), len(c["coords"]), 1 if c["src"] is None else len(c["src"]))[0] > 1 for c in cases)
    seam = kc.span_seam_case()
    assert kc.spans(len(seam["q"]), len(seam["coords"]), 1)[0] == 5 and len(seam["q"]) == kc.TILE_M
    assert max(len(c["coords"]) for c in cases) == len(seam["coords"])


def test_knn_host_equals_the_python_restatement_on_every_case(tables):
    ties = zeros = short = 0
    for case, (idx, d2) in tables:
        want_idx, want_d2 = kc.restate_search(case)
        assert kc.same_table(idx, d2, want_idx, want_d2), (case["q"].shape, case["coords"].shape, case["k"])
        assert idx.dtype == np.int32 and d2.dtype == np.float64
        ties += int(((d2[..., 1:] == d2[..., :-1]) & (idx[..., 1:] >= 0)).sum())
        zeros += int(((d2 == 0) & (idx >= 0)).sum())
        short += int((idx < 0).sum())
        assert ((idx[..., 1:] > idx[..., :-1]) | (d2[..., 1:] > d2[..., :-1]) | (idx[..., 1:] < 0)).all()      # the total order
    print(f"{len(tables)} cases: {ties} tied neighbours, {zeros} zero distances, {short} empty slots")
    assert ties > 1000 and zeros > 100 and short > 100


def test_the_comparator_has_teeth(tables):
    case, (idx, d2) = next((c, t) for c, t in tables if c["k"] >= 2 and len(c["q"]) == 130 and
                           ((t[1][0, :, 0] == t[1][0, :, 1]) & (t[0][0, :, 1] >= 0)).any() and
                           (np.isfinite(t[1]) & (t[1] > 0)).any())
    assert kc.same_table(idx, d2, idx.copy(), d2.copy())
    j = int(np.nonzero((d2[0, :, 0] == d2[0, :, 1]) & (idx[0, :, 1] >= 0))[0][0])
    swapped = idx.copy()
    swapped[0, j, [0, 1]] = idx[0, j, [1, 0]]                    # two tied neighbours swapped
    assert not kc.same_table(swapped, d2, idx, d2)
    at = tuple(int(a[0]) for a in np.nonzero(np.isfinite(d2) & (d2 > 0)))
    ulp = d2.copy()
    ulp[at] = np.nextafter(ulp[at], np.inf)                      # a single d2 one ulp off
    assert not kc.same_table(idx, ulp, idx, d2)
    near, idw = BL.knn_apply_host(idx, d2, case["k"], case["z"], 2)
    assert kc.same_bits(idw, idw.copy()) and kc.same_bits(near, near.copy())
    off = idw.copy()
    t, j = (int(a[0]) for a in np.nonzero(np.isfinite(idw)))
    off[t, j] = np.nextafter(off[t, j], np.float32(np.inf))      # an apply result one float32 ulp off
    assert not kc.same_bits(off, idw)
    nan_moved = idw.copy()
    nan_moved[t, j] = np.nan
    assert not kc.same_bits(nan_moved, idw)


@pytest.mark.parametrize("power", kc.POWERS)
def test_knn_apply_host_against_long_double_sums(tables, power):
    """nearest equal; idw within 0.5 ulp_f32 + (k + 4) 2^-52 sum(w |z|) / sum(w) of the long-double value, NaN and inf
    where it is; also with a prefix k < k_tab of the rows."""
    worst, n = 0.0, 0
    for case, (idx, d2) in tables:
        if len(case["q"]) > 65 and power not in (0, 2):          # (the python loop of the restatement: keep it quick)
            continue
        for k in {case["k"], max(1, case["k"] // 2)}:
            near, idw = BL.knn_apply_host(idx, d2, k, case["z"], power)
            want_near, want, scale = kc.restate_apply(idx, d2, k, case["z"], power)
            assert near.dtype == idw.dtype == np.float32 and kc.same_bits(near, want_near)
            fin = np.isfinite(want.astype(np.float64))
            assert np.array_equal(np.isnan(idw), np.isnan(want.astype(np.float64)))
            assert np.array_equal(idw[~fin & ~np.isnan(idw)], want.astype(np.float32)[~fin & ~np.isnan(idw)])
            ulp = np.spacing(np.abs(want[fin]).astype(np.float32)).astype(np.longdouble)
            bound = 0.5 * ulp + (k + 4) * np.longdouble(2.0 ** -52) * scale[fin]
            err = np.abs(idw[fin].astype(np.longdouble) - want[fin])
            assert (err <= bound).all(), (power, k, float((err / bound).max()))
            if fin.any():
                worst, n = max(worst, float((err / bound).max())), n + int(fin.sum())
    print(f"power {power}: {n} values, worst |delta| / bound = {worst:.4f}")
    assert n > 1000


def test_empty_and_degenerate_shapes():
    idx, d2 = BL.knn_host(np.zeros((0, 2)), np.zeros((5, 2)), None, 3)
    assert idx.shape == (1, 0, 3) and d2.shape == (1, 0, 3)
    idx, d2 = BL.knn_host(np.zeros((4, 2)), np.zeros((0, 2)), None, 3)
    assert (idx == -1).all() and np.isinf(d2).all() and idx.shape == (1, 4, 3)
    near, idw = BL.knn_apply_host(idx, d2, 2, np.zeros((2, 0), dtype=np.float32), 2)
    assert near.shape == (2, 4) and np.isnan(near).all() and np.isnan(idw).all()
    idx, d2 = BL.knn_host(np.zeros((2, 2)), np.zeros((2, 2)), None, 2, exclude_self=True)
    assert np.array_equal(idx[0], [[1, -1], [0, -1]]) and np.array_equal(d2[0], [[0, np.inf], [0, np.inf]])
    for bad in (dict(k=0), dict(k=17), dict(exclude_self=True)):
        with pytest.raises(ValueError):
            BL.knn_host(np.zeros((3, 2)), np.zeros((2, 2)), None, **dict(dict(k=1), **bad))
    with pytest.raises(ValueError):
        BL.knn_apply_host(idx, d2, 3, np.zeros((1, 2), dtype=np.float32), 2)
    with pytest.raises(ValueError):
        BL.knn_apply_host(idx, d2, 1, np.zeros((1, 2), dtype=np.float32), 5)
    # an inf distance is a neighbour like any other, after every finite one; its weight is 0
    c = np.array([[0, 0], [np.inf, 0], [1, 0]], dtype=np.float32)
    idx, d2 = BL.knn_host(np.array([[0.25, 0]], dtype=np.float32), c, None, 3)
    assert np.array_equal(idx[0, 0], [0, 2, 1]) and d2[0, 0, 2] == np.inf
    near, idw = BL.knn_apply_host(idx, d2, 3, np.array([[1, 100, 3]], dtype=np.float32), 2)
    assert near[0, 0] == 1 and idw[0, 0] == np.float32((16.0 + 3 / 0.5625) / (16.0 + 1 / 0.5625))


@pytest.mark.parametrize("n_sites,ny,nx", kc.RASTER_CASES)
def test_raster_and_table_equal_scipy_with_no_node_left_out(n_sites, ny, nx):
    """rasterize_nearest on the host route equals scipy.interpolate.griddata(method="nearest") and knn_host equals
    cKDTree.query's indices, exactly and at EVERY node: the test itself shows that every node's two smallest d2 differ
    by more than 1e-9 relative, so the reference's own float64 search cannot be split by rounding."""
    from scipy.interpolate import griddata
    from scipy.spatial import cKDTree
    case = kc.make_raster_case(n_sites, ny, nx)
    raster, x, y = BL.rasterize_nearest(case["coords"], case["values"], resolution=(ny, nx))
    assert raster.shape == (ny, nx) and raster.dtype == np.float32 and x.dtype == y.dtype == np.float32
    assert np.array_equal(x, np.linspace(0, 1, nx).astype(np.float32)) and len(y) == ny
    xg, yg = np.meshgrid(x.astype(np.float64), y.astype(np.float64))
    nodes = np.stack([xg.reshape(-1), yg.reshape(-1)], axis=1)
    idx, d2 = BL.knn_host(nodes.astype(np.float32), case["coords"], None, 2)
    margin = (d2[0, :, 1] - d2[0, :, 0]) / d2[0, :, 1]
    print(f"{n_sites} sites, {ny} x {nx} nodes: the smallest relative margin between the two nearest is {margin.min():.3e}")
    assert margin.min() > 1e-9
    c64 = case["coords"].astype(np.float64)
    want = griddata(c64, case["values"], (xg, yg), method="nearest")
    assert np.array_equal(raster, want.astype(np.float32))
    dist, tree_idx = cKDTree(c64).query(nodes, k=2)
    assert np.array_equal(idx[0], tree_idx.astype(np.int32))
    assert np.allclose(np.sqrt(d2[0]), dist, rtol=1e-14, atol=0)
    # several rows, one of them with holes: the sources of a row are the sites where it is finite
    rows = np.stack([case["values"], np.where(np.arange(n_sites) % 3 == 0, np.nan, case["values"])]).astype(np.float32)
    many, _, _ = BL.rasterize_nearest(case["coords"], rows, resolution=(ny, nx))
    keep = np.arange(n_sites) % 3 != 0
    holes = griddata(c64[keep], case["values"][keep], (xg, yg), method="nearest")
    assert many.shape == (2, ny, nx) and np.array_equal(many[0], raster)
    idx3, d3 = BL.knn_host(nodes.astype(np.float32), case["coords"][keep], None, 2)
    assert ((d3[0, :, 1] - d3[0, :, 0]) / d3[0, :, 1]).min() > 1e-9
    assert np.array_equal(many[1], holes.astype(np.float32))
    none, _, _ = BL.rasterize_nearest(case["coords"], np.full(n_sites, np.nan), resolution=5, bounds=((0, 1), (0, 2)))
    assert none.shape == (5, 5) and np.isnan(none).all()


def _site_wise(T=7, S=60, seed=4):
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = (np.sin(5 * coords[:, 0])[None, :] + rs.standard_normal((T, S)) * 0.2).astype(np.float32)
    site_code = rs.randint(1, 4, size=S)
    masks = [np.broadcast_to(site_code == c, (T, S)).copy() for c in (1, 2, 3)]
    return coords, z, masks


def test_grid_baselines_shared_and_per_time_routes_agree():
    coords, z, masks = _site_wise()
    for max_rows in (None, 3 * 60):                              # one chunk; chunks of three slices, the last ragged
        shared = BL.grid_baselines(z, coords, *masks, max_rows=max_rows)
        forced = BL.grid_baselines(z, coords, *masks, config={"baseline_per_time": True}, max_rows=max_rows)
        assert shared["shared_table"] and not forced["shared_table"] and shared["k"] == 8 and shared["power"] == 2
        np.testing.assert_equal({k: v for k, v in shared.items() if k != "shared_table"},
                                {k: v for k, v in forced.items() if k != "shared_table"})
    e = shared["idw"]
    assert set(e) == {"splits", "site_mse", "site_mse_by_split", "time_mse"} and set(e["splits"]) == \
        {"all", "train", "valid", "test", "other"}
    assert e["site_mse"].shape == (60,) and e["site_mse_by_split"].shape == (4, 60) and e["time_mse"].shape == (7,)
    assert np.isfinite(e["splits"]["test"]["mse"]) and e["splits"]["other"]["rows"] == 0
    # a field with holes in the training entries: the sources differ by time, so a table per time
    z2 = z.copy()
    z2[2, np.nonzero(masks[0][0])[0][:5]] = np.nan
    assert not BL.grid_baselines(z2, coords, *masks)["shared_table"]
    with pytest.raises(ValueError):
        BL.grid_baselines(z, coords, None)


def test_grid_baselines_constant_slices_and_a_hand_checkable_case():
    coords, z, masks = _site_wise()
    const = np.broadcast_to(np.arange(7, dtype=np.float32)[:, None] * 1.7 + 0.3, z.shape).copy()
    got = BL.grid_baselines(const, coords, *masks)
    for b in ("nearest", "idw"):
        assert all(got[b]["splits"][s]["mse"] == 0.0 for s in ("all", "train", "valid", "test"))
        assert np.array_equal(got[b]["time_mse"], np.zeros(7))
    # five sites on a line at x = 0, 1, 2, 4, 8; train 0, 1, 3; valid 2; test 4; two times, the second 10 x the first
    coords = np.array([[0, 0], [1, 0], [2, 0], [4, 0], [8, 0]], dtype=np.float32)
    z = np.array([[1, 2, 3, 4, 5], [10, 20, 30, 40, 50]], dtype=np.float32)
    site = lambda *s: np.broadcast_to(np.isin(np.arange(5), s), (2, 5)).copy()      # noqa: E731
    got = BL.grid_baselines(z, coords, site(0, 1, 3), site(2), site(4), config={"baseline_k": 2, "baseline_power": 1})
    assert got["shared_table"] and got["k"] == 2 and got["power"] == 1
    assert np.array_equal(got["train_dist"], [1, 1, 1, 3, 4])
    # nearest: 2, 1, 2 (site 1 at distance 1; sites 0 and 3 tie at 2 behind it), 2, 4 against 1 .. 5
    near = got["nearest"]
    assert near["splits"]["train"]["mse"] == 101.0 and near["splits"]["valid"]["mse"] == 50.5
    assert near["splits"]["test"]["mse"] == 50.5 and near["splits"]["train"]["rows"] == 6
    assert np.array_equal(near["site_mse"], np.array([1, 1, 1, 4, 1]) * 50.5)
    assert np.array_equal(near["time_mse"], [8 / 5, 160.0])
    # idw with w = 1 / d over two neighbours: 2.4, 1.75, 5/3 (the tie at distance 2 goes to site 0), 11/7, 36/11
    pred = np.array([2.4, 1.75, 5 / 3, 11 / 7, 36 / 11])
    err2 = (pred - np.arange(1, 6)) ** 2 * 50.5
    assert np.allclose(got["idw"]["site_mse"], err2, rtol=1e-6)
    assert got["idw"]["splits"]["test"]["mse"] == pytest.approx(err2[4], rel=1e-6)
    assert got["idw"]["splits"]["train"]["mse"] == pytest.approx(err2[[0, 1, 3]].mean(), rel=1e-6)


def _cpu_model():
    from stnf.models import STInterpMLP
    torch.manual_seed(3)
    return STInterpMLP(p=0, k_spatial_centers=[25, 81], k_temporal_centers=[10], hidden_dims=[32, 16], dropout=0.0).eval()


def test_grid_scores_baseline_entry_on_a_cpu_model(tmp_path):
    from stnf.utils import grid_baselines, grid_scores, rasterize_nearest, save_grid_scores_npz
    assert grid_baselines is BL.grid_baselines and rasterize_nearest is BL.rasterize_nearest
    m = _cpu_model()
    coords, z, masks = _site_wise()
    z[1, 5] = np.nan
    plain = grid_scores(m, z, coords, *masks)
    again = grid_scores(m, z, coords, *masks, config={"baselines": False})
    got = grid_scores(m, z, coords, *masks, config={"baselines": True, "baseline_k": 4})
    assert "baseline" not in plain and "baseline" not in again and set(got) == set(plain) | {"baseline"}
    np.testing.assert_equal({k: v for k, v in got.items() if k != "baseline"}, plain)
    np.testing.assert_equal(again, plain)
    base = got["baseline"]
    alone = BL.grid_baselines(z, coords, *masks, config={"baseline_k": 4})
    np.testing.assert_equal({k: v for k, v in base.items() if k not in ("skill", "site_skill")}, alone)
    assert base["k"] == 4 and set(base["skill"]) == {"nearest", "idw"} and base["site_skill"].shape == (2, len(coords))
    for r, b in enumerate(("nearest", "idw")):
        for s in ("all", "train", "valid", "test"):
            assert base["skill"][b][s] == 1.0 - plain["splits"][s]["mse"] / base[b]["splits"][s]["mse"]
        assert np.isnan(base["skill"][b]["other"])               # no entry outside the three masks
        with np.errstate(invalid="ignore", divide="ignore"):
            want = 1.0 - plain["site_mse_by_split"][3] / base[b]["site_mse_by_split"][3]
        assert np.array_equal(base["site_skill"][r], want, equal_nan=True)
        assert np.isfinite(base["site_skill"][r]).sum() == int(masks[2][0].sum())
    assert base["skill"]["idw"]["test"] < 0                      # an untrained model is WORSE than the baseline
    path = save_grid_scores_npz(tmp_path, got)
    with np.load(path) as f:
        assert float(f["baseline/idw/splits/test/mse"]) == base["idw"]["splits"]["test"]["mse"]
        assert float(f["baseline/skill/nearest/valid"]) == base["skill"]["nearest"]["valid"]
        assert np.array_equal(f["baseline/train_dist"], base["train_dist"]) and "site_mse" in f.files
        assert np.array_equal(f["baseline/site_skill"], base["site_skill"], equal_nan=True)
