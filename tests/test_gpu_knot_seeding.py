"""k-means++ seeding on the device: stdadk_kmeanspp_f64 against the numpy restatement of its contract and against sklearn.

Kernel against restatement (golden/seed_cases.py, numpy's own sums): on every edge shape every run's seeds equal in
coordinates and pot_out within the summation bound n 2^-52 pot; the same bits twice.  With the restatement's sums formed
in the kernel's order (restate(rows=...)) the rows and the bits of pot_out are equal -- the order written into the
contract is the order the kernel uses.  Degenerate case: duplicated sites with k above the number of distinct points --
from the step whose thresholds are formed on pot == 0 the pick is row 0, nothing is NaN, no sentinel survives.
sklearn's recorded seeds (golden/seed_*.npz and the fits' fixtures) through the kernel: equal in coordinates.
Initialisers: gmm_knots and balanced_kmeans_knots with seeding='device' against 'host' bit for bit; create_model with
spatial_init_seeding.  The equalities are conditions, not tolerances (tests/test_seed_cases_cpu.py shows that no fixed
case is decided by the rounding of a sum)."""
import numpy as np
import pytest
import torch

from golden import cases
from golden import gmm_cases as gc
from golden import kmeans_cases as kc
from golden import seed_cases as sc
from stnf import _native as N
from stnf import knot_init

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run_kernel(X, first, u):
    """One stdadk_kmeanspp_f64 call into poisoned outputs: (rows (runs, k) int64, pots (runs,))."""
    runs, k = u.shape[0], u.shape[1] + 1
    n = len(X)
    Xd, fd, ud = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (X, first, u))
    idx = torch.full((runs, k), -1, device=DEV, dtype=torch.int32)
    pot = torch.full((runs,), float("nan"), device=DEV, dtype=torch.float64)
    ws = torch.full((N.kmeanspp_workspace_bytes(n, k, runs) // 8,), float("nan"), device=DEV, dtype=torch.float64)
    N.kmeanspp(Xd, fd, ud, idx, pot, ws)
    return idx.cpu().numpy().astype(np.int64), pot.cpu().numpy()


def check_against_restatement(name, inp):
    X, n = inp["X"], len(inp["X"])
    want_rows, want_pots, zero = sc.edge_expected(name)
    rows, pots = run_kernel(X, inp["first"], inp["u"])
    assert np.isfinite(pots).all() and rows.min() >= 0 and rows.max() < n, (name, "a sentinel survived", pots, rows.min())
    moved = sc.compare_seeds(X, rows, want_rows, name)
    err = np.abs(pots - want_pots)
    print(f"{name}: L {inp['L']}, rows per thread {sc.rows_per_thread(n)}, {moved} of {rows.size} indices name another row "
          f"of the same site, pot error {err.max():.3e} (bound {sc.pot_bound(n, want_pots).min():.3e})")
    assert (err <= sc.pot_bound(n, want_pots)).all(), (name, pots, want_pots)
    assert np.array_equal(rows[:, 0], np.asarray(inp["first"], np.int64))
    # the sums in the kernel's own order: the same rows, the same bits
    krows, kpots, _ = sc.edge_expected(name, True)
    assert np.array_equal(rows, krows), (name, np.argwhere(rows != krows)[:3])
    assert np.array_equal(pots.view(np.uint64), kpots.view(np.uint64)), (name, pots, kpots)
    again_rows, again_pots = run_kernel(X, inp["first"], inp["u"])
    assert np.array_equal(rows, again_rows) and np.array_equal(pots.view(np.uint64), again_pots.view(np.uint64)), \
        (name, "not the same bits twice")
    return rows, pots, zero


@pytest.mark.parametrize("name", [c["name"] for c in sc.EDGE_CASES])
def test_kernel_reproduces_the_restatement(name):
    check_against_restatement(name, sc.edge_inputs(name))


@pytest.mark.parametrize("name", [c["name"] for c in sc.DEGENERATE_CASES])
def test_more_seeds_than_distinct_points(name):
    inp = sc.degenerate_inputs(name)
    rows, pots, zero = check_against_restatement(name, inp)
    k = rows.shape[1]
    assert inp["distinct"] < k
    for r in range(len(rows)):
        assert zero[r] == inp["distinct"] and (rows[r, zero[r]:] == 0).all() and pots[r] == 0.0, (name, r, rows[r])
        assert len(np.unique(inp["X"][rows[r, :zero[r]]], axis=0)) == inp["distinct"]      # every site once, before


@pytest.mark.parametrize("name", sc.SKLEARN_CASES)
def test_kernel_reproduces_sklearn(name):
    fx = sc.sklearn_case(name)
    rows, pots = run_kernel(fx["X"], fx["first"], fx["u"])
    moved = sc.compare_seeds(fx["X"], rows, fx["seeds"], name)
    print(f"{name}: {moved} of {rows.size} indices name another row of the same site; pots {pots}")
    assert np.isfinite(pots).all() and (pots > 0).all()


def test_device_seeder_equals_the_host_seeder():
    pts = gc.fit_points(gc.FIT_CASES[0])
    levels = [1, 25, 81, 121]
    host = knot_init.kmeanspp_seeds(pts, levels)
    dev = knot_init.kmeanspp_seeds_device(torch.from_numpy(pts).to(DEV), levels)
    for k, h, d in zip(levels, host, dev):
        assert len(d) == knot_init.N_INIT and all(a.shape == (k,) and a.dtype == np.int64 for a in d)
        sc.compare_seeds(pts, np.stack(d), np.stack(h), f"k={k}")
    with pytest.raises(ValueError):
        knot_init.kmeanspp_seeds_device(torch.from_numpy(pts[:20]).to(DEV), [25])


# ---- initialisers -------------------------------------------------------------------------------------------------
def both_ways(fn, coords, levels, np_seed):
    out = []
    for seeding in ("host", "device"):
        np.random.seed(np_seed)
        out.append(fn(coords, levels, DEV, seeding=seeding))
    return out


def test_gmm_knots_device_seeding_equals_host_seeding():
    case = gc.MODULE_CASE
    (hc, hb), (dc, db) = both_ways(knot_init.gmm_knots, gc.module_coords(case), case["n_centers"], case["np_seed"])
    assert hc.shape == (sum(case["n_centers"]), 2) and torch.equal(hc, dc) and torch.equal(hb, db)


@pytest.mark.parametrize("name", [c["name"] for c in kc.FIT_CASES])
def test_balanced_kmeans_knots_device_seeding_equals_host_seeding(name):
    case = next(c for c in kc.FIT_CASES if c["name"] == name)
    (hc, hb), (dc, db) = both_ways(knot_init.balanced_kmeans_knots, kc.fit_points(case), [case["k"]], 5)
    assert hc.shape == (case["k"], 2) and torch.equal(hc, dc) and torch.equal(hb, db)


def test_create_model_reads_spatial_init_seeding():
    from stnf.models import create_model
    pts = cases.init_points()[::3]             # 1000 clustered rows with duplicates, float32
    config = dict(k_spatial_centers=[25, 81], k_temporal_centers=[5], hidden_dims=[16], spatial_init_method='gmm',
                  spatial_init_device=DEV)
    models = []
    for extra in ({}, dict(spatial_init_seeding='host'), dict(spatial_init_seeding='device')):
        np.random.seed(5)
        models.append(create_model(dict(config, **extra), train_coords=pts).spatial_basis)
    for m in models[1:]:
        assert torch.equal(m.centers, models[0].centers) and torch.equal(m.bandwidths, models[0].bandwidths)
    # the device seeder was the one that ran
    calls = []
    orig = knot_init.kmeanspp_seeds_device
    knot_init.kmeanspp_seeds_device = lambda *a, **kw: calls.append(1) or orig(*a, **kw)
    try:
        np.random.seed(5)
        create_model(dict(config, spatial_init_seeding='device'), train_coords=pts)
        assert calls == [1]
        np.random.seed(5)
        create_model(config, train_coords=pts)
        assert calls == [1]
    finally:
        knot_init.kmeanspp_seeds_device = orig
    with pytest.raises(ValueError):
        create_model(dict(config, spatial_init_seeding='device', spatial_init_device=None), train_coords=pts)
    with pytest.raises(ValueError):
        create_model(dict(config, spatial_init_seeding='cuda'), train_coords=pts)
