"""Basis diagnostics, the half that runs anywhere: the restatements of stnf.utils.basis_diag agree with each other and
stay within a quarter of the comparator's bound of the long-double restatement (tests/golden/basis_diag_cases.py), the
comparator reports what it must, the boundary cases land where stated, the host summaries give their known answers on
a hand-made table, and a `device: cpu` model goes through stnf.utils.basis_diagnostics, grid_scores' `basis` entry
and save_basis_info_npz."""
import os
import re

import numpy as np
import pytest
import torch

from golden import basis_diag_cases as bc
from stnf.utils import basis_diag as BD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "st-dadk_amd", "csrc", "basis_diag.hip")).read()
    val = {"kWave": 64}
    for name, expr in re.findall(r"constexpr int (BD_\w+) = ([\w\s*/+-]+);", src):
        if "STDADK" not in expr:
            val[name] = int(eval(expr, {}, val))
    for name, want in (("BD_Q", bc.WAVES), ("BD_KT", bc.TILE_K), ("BD_SC", bc.CHUNK_S), ("BD_SS", bc.STAGE_S),
                       ("BD_MAX_SPANS", bc.MAX_SPANS), ("BD_ST", bc.TILE_S), ("BD_KC", bc.CHUNK_K), ("BD_KQ", bc.QUARTER_K)):
        assert val[name] == want, name
    assert BD.CAL == bc.CAL and (BD.K_NEAR2, BD.S_NEAR2) == (bc.K_NEAR2, bc.S_NEAR2)
    for S in bc.SIZES_S:
        assert S <= 1100
    assert max(bc.SIZES_K) <= 700


def test_cases_cover_what_they_must():
    for basis in bc.BASES:
        cases = bc.all_cases(basis)
        assert {c["coords"].shape[0] for c in cases} >= set(bc.SIZES_S)
        assert {c["centers"].shape[0] for c in cases} >= set(bc.SIZES_K)
        assert {(c["w"] is None, c["v"] is None) for c in cases} == {(a, b) for a in (True, False) for b in (True, False)}
        assert any(c["sizes"] == (25, 81, 121) for c in cases) and any(c["sizes"][:2] == (3, 70) for c in cases)
        assert any(len(c["sizes"]) == 1 for c in cases)
        assert any(c["w"] is not None and np.isnan(c["w"]).any() and (c["w"] < 0).any() and (c["w"] == 0).any()
                   for c in cases)
        assert any(c["v"] is not None and np.isnan(c["v"]).any() for c in cases)
        big = [c for c in cases if c["coords"].shape[0] >= 9]
        assert all((c["coords"][1] == c["coords"][0]).all() for c in big)
        # sites ON knots: d2 = 0 occurs
        assert all(BD.basis_diag_sums_host(*bc.call_args(c))[1][:, :, bc.S_NEAR2].min() == 0.0 for c in big)


@pytest.mark.parametrize("basis", bc.BASES)
def test_vectorised_and_exact_restatements_agree_and_the_bound_has_room(basis):
    """On every case: the plain-loop statement against the vectorised one by the comparator (N, COVER, NEAR2 equal), and
    the vectorised float64 one within ONE QUARTER of the bound of the long-double one; the recorded figure holds."""
    worst = 0.0
    for case in bc.all_cases(basis):
        rk, rsite, aux = bc.restate_longdouble(case)
        vec = BD.basis_diag_sums_host(*bc.call_args(case))
        bad, ratio = bc.compare(*vec, rk, rsite, aux, fraction=0.25)
        assert not bad, (case["coords"].shape, case["centers"].shape, bad[:3])
        worst = max(worst, ratio)
        ex = BD.restate_exact(*bc.call_args(case))
        bad, _ = bc.compare(*ex, *vec, aux, fraction=0.5)
        assert not bad, (case["coords"].shape, case["centers"].shape, bad[:3])
        for a, b, slots in ((ex[0], vec[0], [bc.K_N, bc.K_NEAR2]), (ex[1], vec[1], [bc.S_COVER, bc.S_NEAR2])):
            assert np.array_equal(a[..., slots], b[..., slots])
        if case["v"] is None:
            assert not vec[0][:, [bc.K_SV, bc.K_WV]].any()
        # a block size that is no divisor changes no decision
        blk = BD.basis_diag_sums_host(*bc.call_args(case), block=37)
        assert not bc.compare(*blk, *vec, aux, fraction=0.5)[0]
    rec = bc.achieved()["worst_ratio"][basis]
    print(f"{basis}: worst |float64 - long double| / bound = {worst:.4f} (recorded {rec:.4f})")
    assert worst <= 0.25 and rec <= 0.25 and abs(worst - rec) <= 0.02


def test_the_recorded_tie_gaps_are_what_the_oracle_shows():
    rec = bc.achieved()["tie_oracle_gap"]
    for basis in bc.BASES:
        gap = bc.tie_oracle_gap(basis)
        assert 0 < gap < 2e-6 and abs(gap - rec[basis]) <= 0.05 * rec[basis], (basis, gap, rec[basis])
        edge = bc.tie_edge_knots(bc.tie_case(basis))
        assert edge.sum() <= 0.02 * len(edge)


def test_the_comparator_has_teeth():
    case = next(c for c in bc.all_cases("wendland")
                if c["w"] is not None and c["v"] is not None and len(c["sizes"]) > 1 and len(c["coords"]) > 100)
    rk, rsite, aux = bc.restate_longdouble(case)
    good = BD.basis_diag_sums_host(*bc.call_args(case))
    assert not bc.compare(*good, rk, rsite, aux)[0]
    # one pair moved across a boundary: a knot's count and a site's cover are off by one
    k = int(np.argmax(good[0][:, bc.K_WV] > 0))
    moved = good[0].copy()
    moved[k, bc.K_N] -= 1
    bad, _ = bc.compare(moved, good[1], rk, rsite, aux)
    assert len(bad) == 1 and bad[0].startswith(f"knot[{k}, {bc.K_N}]")
    i, l = [int(a[0]) for a in np.nonzero(good[1][:, :, bc.S_COVER] > 0)]
    moved = good[1].copy()
    moved[i, l, bc.S_COVER] += 1
    bad, _ = bc.compare(good[0], moved, rk, rsite, aux)
    assert len(bad) == 1 and bad[0].startswith(f"site[{i}, {l}, {bc.S_COVER}]")
    # a minimum off by one ulp
    near = good[0].copy()
    near[k, bc.K_NEAR2] = np.nextafter(near[k, bc.K_NEAR2], np.inf)
    assert len(bc.compare(near, good[1], rk, rsite, aux)[0]) == 1
    # one sum perturbed by twice its bound, each kind of sum in turn
    bk, bs = bc.bounds(rk, rsite, aux)
    for slot in (bc.K_W, bc.K_SPHI, bc.K_SPHI2, bc.K_SV, bc.K_WV):
        off = np.asarray(rk, dtype=np.float64).copy()
        assert bk[k, slot] > 0
        off[k, slot] += 2 * bk[k, slot]
        got = good[0].copy()
        got[:, slot] = off[:, slot]
        bad, _ = bc.compare(got, good[1], rk, rsite, aux)
        assert len(bad) == 1 and bad[0].startswith(f"knot[{k}, {slot}]"), (slot, bad)
    got = good[1].copy()
    got[i, l, bc.S_SPHI] = float(rsite[i, l, bc.S_SPHI]) - 2 * bs[i, l, bc.S_SPHI]
    assert len(bc.compare(good[0], got, rk, rsite, aux)[0]) == 1
    # one swapped level
    swapped = good[1].copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    assert len(case["sizes"]) >= 2 and bc.compare(good[0], swapped, rk, rsite, aux)[0]


def test_boundary_cases_land_where_stated():
    case, want = bc.dyadic_boundary_case()
    assert float(case["coords"][0, 0]) == 0.25 and float(case["coords"][2, 0]) < 0.25
    assert float(np.nextafter(case["coords"][2, 0], np.float32(1))) == 0.25
    for build in (BD.basis_diag_sums_host, BD.restate_exact):
        knot, site = build(*bc.call_args(case))
        assert np.array_equal(site[:, 0, bc.S_COVER], want.astype(np.float64))
        assert knot[0, bc.K_N] == want.sum() and knot[0, bc.K_NEAR2] == 0.0
        # at the strict edge phi would be 0 anyway; one float32 below it, it is tiny and positive
        assert 0 < site[2, 0, bc.S_SPHI] < 1e-40 and site[0, 0, bc.S_SPHI] == 0 and site[4, 0, bc.S_SPHI] == 1.0
    for basis in ("triangular", "gaussian"):
        case, want = bc.searched_boundary_case(basis)
        for build in (BD.basis_diag_sums_host, BD.restate_exact):
            knot, site = build(*bc.call_args(case))
            assert np.array_equal(site[:, 0, bc.S_COVER], want.astype(np.float64)), basis
            assert knot[0, bc.K_N] == 3
        if basis == "gaussian":                                   # the tail beyond rho is dropped by contract
            assert site[1, 0, bc.S_SPHI] == 0 and 4e-5 < site[0, 0, bc.S_SPHI] < 5e-5


def test_host_summaries_known_answers():
    # sparsity analysis: norms 0, 0.005, 0.5, 1, 2 -> threshold 0.02 at ratio 1e-2
    norms = np.array([0.0, 0.005, 0.5, 1.0, 2.0])
    sp = BD.sparsity_summary(norms ** 2)
    assert np.allclose(sp["norms"], norms, rtol=1e-15) and sp["threshold"] == pytest.approx(0.02)
    assert sp["inactive"].tolist() == [True, True, False, False, False] and (sp["n_inactive"], sp["n_active"]) == (2, 3)
    assert np.allclose(sp["percentile_values"], np.percentile(norms, [10, 25, 50, 75, 90]))
    assert np.allclose(sp["percentile_values"], [0.002, 0.005, 0.5, 1.0, 1.6])
    assert sp["small_counts"].tolist() == [1, 2, 2] and sp["norm_median"] == 0.5 and sp["norm_mean"] == pytest.approx(0.701)
    assert BD.sparsity_summary(norms ** 2, ratio=0.3)["inactive"].tolist() == [True, True, True, False, False]
    zero = BD.sparsity_summary(np.zeros(4))
    assert zero["threshold"] == 0.0 and not zero["inactive"].any() and zero["n_active"] == 4
    # movement: 3-4-5 triangles
    init = np.array([[0.0, 0.0], [0.5, 0.5], [1.0, 1.0], [0.2, 0.2]])
    final = init + np.array([[0.3, 0.4], [0.0, 0.0], [0.06, 0.08], [-0.6, -0.8]])
    mv = BD.movement_summary(init, final)
    assert np.allclose(mv["movement"], [0.5, 0.0, 0.1, 1.0])
    assert (mv["movement_mean"], mv["movement_max"], mv["movement_median"]) == pytest.approx((0.4, 1.0, 0.3))
    act = BD.movement_summary(init, final, inactive=np.array([False, False, False, True]))
    assert (act["movement_mean"], act["movement_max"], act["movement_median"]) == pytest.approx((0.2, 0.5, 0.1))
    none = BD.movement_summary(init, final, inactive=np.ones(4, dtype=bool))
    assert (none["movement_mean"], none["movement_max"], none["movement_median"]) == (0.0, 0.0, 0.0)
    # out of domain: knots 2 (1.06, 1.08) and 3 (-0.4, -0.6)
    n, mask = BD.out_of_domain(final)
    assert n == 2 and mask.tolist() == [False, False, True, True]
    # path length: out and back is twice the way, the movement is 0
    mid = init + np.array([[0.3, 0.4]] * 4)
    assert np.allclose(BD.path_length(init, [(100, mid)], init), 1.0)
    assert np.allclose(BD.path_length(init, [(100, mid), (200, final)], final),
                       0.5 + np.linalg.norm(final - mid, axis=1))
    assert np.allclose(BD.path_length(init, None, final), mv["movement"])
    # per-level bandwidths
    st = BD.level_bandwidth_stats([1.0, 3.0, 2.0, 2.0, 2.0], [2, 3])
    assert st["level_bw_mean"].tolist() == [2.0, 2.0] and st["level_bw_std"].tolist() == [1.0, 0.0]
    assert st["level_bw_min"].tolist() == [1.0, 2.0] and st["level_bw_max"].tolist() == [3.0, 2.0]
    # temporal support: one knot at 0 with bw 1, times 0 and 1, weights 2 and 3
    assert BD.temporal_support([0.0], [1.0], [0.0, 1.0], [2, 3])[0] == pytest.approx(2 + 3 * np.exp(-0.5))
    # group norms
    W = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert BD.group_sumsq_host(W, 1, 2).tolist() == [1 + 25 + 81, 4 + 36 + 100]
    # dead knots and uncovered sites from the accumulators
    case, _ = bc.dyadic_boundary_case()
    knot, site = BD.basis_diag_sums_host(*bc.call_args(case))
    out = BD.summarize(knot, site, case["sizes"], case["centers"], case["bw"])
    assert out["dead"].tolist() == [False] and out["uncovered"][:, 0].tolist() == [True, True, False, False, False, True,
                                                                                 True, False]
    assert out["level_uncovered"].tolist() == [4] and out["knot_nearest"][0] == 0.0
    far = BD.summarize(*BD.basis_diag_sums_host(case["centers"], case["bw"], "wendland", (1,), [[0.9, 0.9]]), (1,),
                       case["centers"], case["bw"])
    assert far["dead"].tolist() == [True] and far["n_dead"] == 1 and np.isnan(far["knot_value"][0])


def _cpu_model():
    from stnf.models import STInterpMLP
    torch.manual_seed(3)
    return STInterpMLP(p=0, k_spatial_centers=[25, 81], k_temporal_centers=[10], hidden_dims=[32, 16], dropout=0.0,
                       spatial_learnable=True).eval()


def _field(S=40, T=6):
    rs = np.random.RandomState(8)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = rs.standard_normal((T, S)).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.1] = np.nan
    code = rs.randint(0, 4, size=(T, S))
    return coords, z, [code == c for c in (1, 2, 3)]


def test_cpu_model_route(tmp_path):
    import copy
    from stnf.utils import basis_diagnostics, grid_scores, save_basis_info_npz, save_grid_scores_npz
    m = _cpu_model()
    initial = copy.deepcopy(m)
    with torch.no_grad():
        m.spatial_basis.centers[3] += torch.tensor([0.3, 0.4])
        m._body[0].weight[:, 7] = 0.0
    coords, z, masks = _field()
    sse = np.arange(len(coords), dtype=np.float64)
    d = basis_diagnostics(m, coords, train_mask=masks[0], config={"sparsity_threshold_ratio": 1e-2}, model_initial=initial,
                          history=[(100, initial.spatial_basis.centers.detach().numpy())], site_value=sse)
    w = masks[0].sum(axis=0).astype(np.float64)
    knot, site = BD.restate_exact(m.spatial_basis.centers.detach().numpy(), m.spatial_basis.bandwidths.detach().numpy(),
                                  "wendland", (25, 81), coords, w, sse)
    assert np.array_equal(d["knot_count"], knot[:, bc.K_N]) and np.array_equal(d["site_cover"], site[:, :, bc.S_COVER])
    assert np.allclose(d["knot_sphi"], knot[:, bc.K_SPHI], rtol=1e-13) and np.array_equal(d["site_weight"], w)
    assert d["movement"][3] == pytest.approx(0.5, rel=1e-6) and d["movement_max"] == pytest.approx(0.5, rel=1e-6)
    assert d["path_length"][3] == pytest.approx(0.5, rel=1e-6) and d["inactive"][7] and d["sparsity_n_inactive"] == 1
    assert d["out_of_domain"] == int(((m.spatial_basis.centers < 0) | (m.spatial_basis.centers > 1)).any(1).sum())
    assert d["level_bw_mean"].shape == (2,) and d["temporal_support"].shape == (10,) and d["rho"] == 1.0
    assert d["uncovered"].shape == (len(coords), 2) and d["dead"].shape == (106,)
    # grid_scores: the entry with the key, key for key what it was without
    plain = grid_scores(m, z, coords, *masks)
    again = grid_scores(m, z, coords, *masks, config={"basis_diagnostics": False})
    got = grid_scores(m, z, coords, *masks, config={"basis_diagnostics": True})
    assert "basis" not in plain and set(got) == set(plain) | {"basis"}
    np.testing.assert_equal({k: v for k, v in got.items() if k != "basis"}, plain)
    np.testing.assert_equal(again, plain)
    assert np.array_equal(got["basis"]["knot_count"], d["knot_count"])
    assert np.array_equal(got["basis"]["site_cover"], d["site_cover"])
    path = save_grid_scores_npz(tmp_path, got)
    with np.load(path) as f:
        assert np.array_equal(f["basis/knot_count"], d["knot_count"]) and "site_mse" in f.files
    # basis_info.npz: the reference's eight keys and the diagnostics
    path = save_basis_info_npz(tmp_path, d, initial, m)
    with np.load(path) as f:
        assert set(BD.BASIS_INFO_KEYS) <= set(f.files) and len(BD.BASIS_INFO_KEYS) == 8
        assert np.array_equal(f["spatial_centers_init"], initial.spatial_basis.centers.detach().numpy())
        assert np.array_equal(f["spatial_centers_final"], m.spatial_basis.centers.detach().numpy())
        assert np.array_equal(f["spatial_bandwidths_final"], m.spatial_basis.bandwidths.detach().numpy())
        assert np.array_equal(f["temporal_centers_init"], m.temporal_basis.centers.numpy())
        assert np.array_equal(f["diag/dead"], d["dead"]) and np.array_equal(f["diag/movement"], d["movement"])
