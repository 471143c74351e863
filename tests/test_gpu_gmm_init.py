"""The knot initialiser on the device: stdadk_gmm_em_f64 alone against the float64 restatement of golden/gmm_cases.py
(bound: K_FACTOR x what two summation orders of the restatement disagree by, golden/gmm_achieved.json) and its
determinism; stnf.knot_init.fit_spherical_gmm against sklearn's recorded fits (golden/gmm_fit_*.npz: the discrete
decisions equal, the values within K_FACTOR x the restatement's own disagreement D with sklearn); the module and
create_model with init_device / spatial_init_device against the reference's recorded _init_gmm (golden/gmm_module_*.npz).
The fixtures carry the k-means++ seeds of the fit cases; neither the reference nor the restatement's fit runs here."""
import functools
import os

import numpy as np
import pytest
import torch

from golden import gmm_cases as gc
from stnf import _native as N
from stnf import knot_init

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """(inputs, float64 reference) of a one-iteration case, computed once."""
    case = next(c for c in gc.ITER_CASES if c["name"] == name)
    inp = gc.iter_inputs(case)
    return case, inp, gc.em_iteration(inp["X"], inp["w"], inp["mu"], inp["var"], order="pairwise")


def run_em(inp, reg_covar=gc.REG_COVAR):
    """One stdadk_gmm_em_f64 call into NaN-filled outputs: dict(w, mu, var, lb) as numpy."""
    X, w, mu, var = (torch.from_numpy(np.ascontiguousarray(inp[a])).to(DEV) for a in ("X", "w", "mu", "var"))
    n, k = X.shape[0], w.shape[0]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=torch.float64)       # noqa: E731
    w2, mu2, var2, lb = nan(k), nan(k, 2), nan(k), nan(1)
    ws = nan(N.gmm_workspace_bytes(n, k) // 8)
    N.gmm_em(X, w, mu, var, reg_covar, w2, mu2, var2, lb, ws)
    return dict(w=w2.cpu().numpy(), mu=mu2.cpu().numpy(), var=var2.cpu().numpy(), lb=float(lb.item()))


@pytest.mark.parametrize("name", [c["name"] for c in gc.ITER_CASES])
def test_one_iteration_matches_the_restatement(name):
    case, inp, ref = evaluated(name)
    got = run_em(inp)
    dis = gc.compare_iteration(got, ref, name)
    print(f"{name}: {gc.fmt(dis)}  (bounds {gc.bounds()})")
    again = run_em(inp)
    for o in ("w", "mu", "var"):
        assert np.array_equal(got[o].view(np.uint64), again[o].view(np.uint64)), (name, o, "not the same bits twice")
    assert np.float64(got["lb"]).view(np.uint64) == np.float64(again["lb"]).view(np.uint64), (name, "lb")
    if case["special"] == "massless":
        j = case["k"] - 1
        assert np.all(ref["mu"][j] == 0.0) and ref["var"][j] == gc.REG_COVAR          # no sample reaches it: r == 0 exactly
        assert np.isfinite(got["w"][j]) and got["w"][j] > 0.0 and np.isfinite(got["var"][j])
        assert np.all(got["mu"][j] == 0.0), got["mu"][j]
        assert got["var"][j] == gc.REG_COVAR, got["var"][j]
    if case["special"] == "on_point":
        assert got["var"][0] >= gc.REG_COVAR


def test_more_components_than_samples_and_every_kernel_edge_is_in_the_list():
    """The list holds n < k, the sample workgroup's, the component tile's and the slab count's edges."""
    shapes = set(gc.ITER_SHAPES)
    assert any(n < k for n, k in shapes)
    for n in (gc.GMM_T - 1, gc.GMM_T, gc.GMM_T + 1):
        assert any(s[0] == n for s in shapes), n
    for k in (gc.GMM_KT - 1, gc.GMM_KT, gc.GMM_KT + 1):
        assert any(s[1] == k for s in shapes), k
    counts = {gc.slabs(n, k)[0] for n, k in shapes}
    assert {1, 2, 3, gc.GMM_MAX_SLABS - 1, gc.GMM_MAX_SLABS} <= counts, sorted(counts)
    assert N.gmm_workspace_bytes(10000, 121) == 8 * (10000 + 40 + 121 * gc.slabs(10000, 121)[0] * 4)


# ---- whole fit --------------------------------------------------------------------------------------------------
def fixture(name):
    return np.load(os.path.join(gc.HERE, f"gmm_{name}.npz"))


@pytest.mark.parametrize("name", [c["name"] for c in gc.FIT_CASES])
def test_fit_reproduces_sklearn(name):
    case = next(c for c in gc.FIT_CASES if c["name"] == name)
    fx = fixture(name)
    k = case["k"]
    fit = knot_init.fit_spherical_gmm(torch.from_numpy(fx["X"]).to(DEV), k, list(fx["seeds"]), max_iter=gc.MAX_ITER,
                                      tol=gc.TOL, reg_covar=gc.REG_COVAR)
    assert list(fit.n_iter) == fx["re_n_iter"].tolist(), (name, fit.n_iter, fx["re_n_iter"])
    assert fit.best == int(fx["re_best"]) and fit.n_iter[fit.best] == int(fx["n_iter"])
    got = dict(w=fit.weights.cpu().numpy(), mu=fit.means.cpu().numpy(), var=fit.variances.cpu().numpy())
    sk = dict(w=fx["weights"], mu=fx["means"], var=fx["covariances"])
    dis, D = gc.fit_disagreement(got, sk), gc.achieved()["fit"][name]["D"]
    print(f"{name}: n_iter {fit.n_iter} best {fit.best}; against sklearn {dis}; D {D}; lb {fit.lower_bound!r} "
          f"(sklearn {float(fx['lower_bound'])!r})")
    for o in ("mu", "var", "w"):
        assert dis[o] <= gc.K_FACTOR * D[o], (name, o, dis[o], "D", D[o])
    c_got, b_got = knot_init.knots_from_fit(got["mu"], got["var"], k)
    c_ref, b_ref = gc.knots32(sk["mu"], sk["var"], k)
    assert gc.ulps32(c_got.numpy(), c_ref) <= 1.0 and gc.ulps32(b_got.numpy(), b_ref) <= 1.0


# ---- module -----------------------------------------------------------------------------------------------------
def assert_knots(centers, bandwidths, fx, rows=None):
    c, b = centers.detach().cpu().numpy(), bandwidths.detach().cpu().numpy()
    rows = slice(None) if rows is None else rows
    uc, ub = gc.ulps32(c, fx["centers"][rows]), gc.ulps32(b, fx["bandwidths"][rows])
    print(f"centres {uc:.2f} ulp, bandwidths {ub:.2f} ulp")
    assert uc <= 1.0 and ub <= 1.0, (uc, ub)


def test_module_with_init_device_matches_the_reference():
    from stnf.models.st_interp import SpatialBasisEmbedding
    fx = fixture(gc.MODULE_CASE["name"])
    assert len(fx["coords"]) > knot_init.MAX_SAMPLES                    # the subsample is drawn
    np.random.seed(int(fx["np_seed"]))
    emb = SpatialBasisEmbedding(n_centers=fx["n_centers"].tolist(), init_method='gmm', train_coords=fx["coords"],
                                init_device=DEV)
    assert emb.centers.dtype == torch.float32 and emb.centers.shape == (106, 2) and not emb.centers.is_cuda
    assert_knots(emb.centers, emb.bandwidths, fx)


def test_create_model_reads_spatial_init_device():
    from stnf.models import create_model
    fx = fixture(gc.MODULE_CASE["name"])
    config = dict(k_spatial_centers=fx["n_centers"].tolist(), k_temporal_centers=[5], hidden_dims=[16],
                  spatial_init_method='gmm', spatial_learnable=True, spatial_init_device=DEV)
    np.random.seed(int(fx["np_seed"]))
    m = create_model(config, train_coords=fx["coords"])
    assert_knots(m.spatial_basis.centers, m.spatial_basis.bandwidths, fx)
    # any other initialiser ignores the key
    u = create_model(dict(config, spatial_init_method='uniform'))
    v = create_model(dict(k_spatial_centers=config["k_spatial_centers"], k_temporal_centers=[5], hidden_dims=[16]))
    assert torch.equal(u.spatial_basis.centers, v.spatial_basis.centers)


def test_without_the_key_the_host_path_runs():
    """The coarse level alone (the levels are fitted one by one on the same subsample): sklearn on the host, as before."""
    from stnf.models import create_model
    fx = fixture(gc.MODULE_CASE["name"])
    k0 = int(fx["n_centers"][0])
    calls = []
    orig = knot_init.gmm_knots
    knot_init.gmm_knots = lambda *a, **kw: calls.append(a) or orig(*a, **kw)
    try:
        np.random.seed(int(fx["np_seed"]))
        m = create_model(dict(k_spatial_centers=[k0], k_temporal_centers=[5], hidden_dims=[16],
                              spatial_init_method='gmm'), train_coords=fx["coords"])
    finally:
        knot_init.gmm_knots = orig
    assert not calls
    assert_knots(m.spatial_basis.centers, m.spatial_basis.bandwidths, fx, rows=slice(0, k0))
