"""The balanced k-means knot initialiser on the device.

E-step: stdadk_kmeans_balanced_iter_f64, one iteration per case of golden/kmeans_cases.py -- labels in range, counts within
[lo, hi] exactly, the host-recomputed float64 cost of the device's labels within B = 16 (n + k) 2^-53 n max c of the
optimum that scipy.optimize.linear_sum_assignment finds (costs compared, never labels), status 0, the same bits twice.
M-step: mu_out, inertia and shift against the restatement on the device's own labels, within n 2^-52 relative.
Fit: stnf.knot_init.fit_balanced_kmeans against golden/kmeans_fit_*.npz (written by the restatement): per-restart
n_iter and the chosen restart equal, centres within 1e-9, every restart's inertia sequence non-increasing up to B.
Module: SpatialBasisEmbedding / create_model with init_device / spatial_init_device, the bandwidths bit for bit the shared
helper's, the forward against the host path (random_site unchanged by the shared helper: tests/test_kmeans_cases_cpu.py)."""
import functools
import os

import numpy as np
import pytest
import torch

from golden import cases
from golden import kmeans_cases as kc
from stnf import _native as N
from stnf import knot_init

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5                 # tests/test_gpu_parity.py: the scattered-knot forward against float64


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """(case, inputs, float64 costs, the oracle's optimum) of a one-iteration case, computed once."""
    case = next(c for c in kc.CASES if c["name"] == name)
    inp = kc.case_inputs(case)
    c = kc.costs(inp["X"], inp["mu"])
    return case, inp, c, kc.oracle(c, inp["lo"], inp["hi"])[0]


def run_iter(inp):
    """One stdadk_kmeans_balanced_iter_f64 call into poisoned outputs: dict(labels, mu, inertia, shift, status)."""
    X, mu = (torch.from_numpy(np.ascontiguousarray(inp[a])).to(DEV) for a in ("X", "mu"))
    n, k = X.shape[0], mu.shape[0]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=torch.float64)       # noqa: E731
    mu2, stats, ws = nan(k, 2), nan(2), nan(N.kmeans_workspace_bytes(n, k) // 8)
    labels = torch.full((n,), -7, device=DEV, dtype=torch.int32)
    status = torch.full((2,), -7, device=DEV, dtype=torch.int32)
    N.kmeans_balanced_iter(X, mu, inp["lo"], inp["hi"], mu2, labels, stats, status, ws)
    st = stats.cpu().numpy()
    return dict(labels=labels.cpu().numpy(), mu=mu2.cpu().numpy(), inertia=float(st[0]), shift=float(st[1]),
                status=status.cpu().numpy())


@pytest.mark.parametrize("name", [c["name"] for c in kc.CASES])
def test_one_iteration_reaches_the_optimum(name):
    case, inp, c, optimum = evaluated(name)
    n, k = case["n"], case["k"]
    got = run_iter(inp)
    assert got["status"][0] == 0, (name, got["status"])
    gap = kc.compare_assignment(got["labels"], c, inp["lo"], inp["hi"], optimum, name)
    print(f"{name}: lo {inp['lo']} hi {inp['hi']} augmentations {got['status'][1]} cost gap {gap:.3e} "
          f"(B {kc.bound_B(n, k, float(c.max())):.3e})")
    assert 0 <= got["status"][1] <= n
    # M-step on the device's own labels
    labels = got["labels"].astype(np.int64)
    rel = n * 2.0 ** -52
    ref_mu = kc.m_step(inp["X"], labels, k)
    ref_inertia = kc.assignment_cost(c, labels)
    ref_shift = float(((ref_mu - inp["mu"]) ** 2).sum())
    assert np.abs(got["mu"] - ref_mu).max() <= rel * max(np.abs(ref_mu).max(), np.abs(inp["X"]).max()), name
    assert abs(got["inertia"] - ref_inertia) <= rel * ref_inertia, (name, got["inertia"], ref_inertia)
    # shift = sum_j |d_j|^2 with d_j = mu_out_j - mu_j: beside the sum's own rel x shift, what the means' error above
    # (e = rel x S per coordinate, S the largest coordinate) does to it: 2 k coordinates x (2 |d| e + e^2)
    e, d = rel * np.abs(inp["X"]).max(), np.abs(ref_mu - inp["mu"]).max()
    assert abs(got["shift"] - ref_shift) <= rel * ref_shift + 2 * k * (2 * d * e + e * e), (name, got["shift"], ref_shift)
    again = run_iter(inp)
    assert np.array_equal(got["labels"], again["labels"]) and np.array_equal(got["status"], again["status"]), name
    assert np.array_equal(got["mu"].view(np.uint64), again["mu"].view(np.uint64)), (name, "mu: not the same bits twice")
    assert np.float64(got["inertia"]).view(np.uint64) == np.float64(again["inertia"]).view(np.uint64)
    assert np.float64(got["shift"]).view(np.uint64) == np.float64(again["shift"]).view(np.uint64)
    if case["special"] in ("far", "far8"):
        far = 8 if case["special"] == "far8" else 1
        assert (np.bincount(labels, minlength=k)[-far:] == inp["lo"]).all()       # filled to lo, no further


def test_every_kernel_edge_is_in_the_case_table():
    assert kc.kernel_constants() == dict(KM_T=kc.KM_T, KM_KT=kc.KM_KT, KM_AT=kc.KM_AT, KM_MAX_K=kc.KM_MAX_K)
    ns, ks = {c["n"] for c in kc.CASES}, {c["k"] for c in kc.CASES}
    for e in (kc.KM_T, kc.KM_AT):
        assert {e - 1, e, e + 1} <= ns, e
    assert {kc.KM_KT - 1, kc.KM_KT, kc.KM_KT + 1, kc.KM_AT // 2, kc.KM_AT // 2 + 1, kc.KM_MAX_K, 1} <= ks
    assert any(c["n"] == c["k"] for c in kc.CASES) and any(c["n"] % c["k"] == 0 and c["k"] > 1 for c in kc.CASES)


# ---- whole fit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in kc.FIT_CASES])
def test_fit_reproduces_the_restatement(name):
    case = next(c for c in kc.FIT_CASES if c["name"] == name)
    fx = np.load(os.path.join(kc.HERE, f"kmeans_{name}.npz"))
    k, X = case["k"], fx["X"]
    history = []
    fit = knot_init.fit_balanced_kmeans(torch.from_numpy(X).to(DEV), k, list(fx["seeds"]), max_iter=kc.MAX_ITER,
                                        tol_factor=kc.TOL_FACTOR, history=history)
    print(f"{name}: n_iter {fit.n_iter} best {fit.best} inertias {fit.inertias}; augmentations per iteration "
          f"{[[h[2] for h in r] for r in history]}")
    assert list(fit.n_iter) == fx["n_iter"].tolist(), (name, fit.n_iter, fx["n_iter"])
    assert fit.best == int(fx["best"])
    err = np.abs(fit.centers.cpu().numpy() - fx["centers"]).max()
    assert err <= kc.CENTRE_TOL, (name, err)
    lo, hi = kc.bounds(len(X), k)
    cnt = np.bincount(fit.labels.cpu().numpy(), minlength=k)
    assert cnt.min() >= lo and cnt.max() <= hi and cnt.sum() == len(X)
    # what an exact E-step guarantees and a heuristic one does not: the inertia never rises.  max c <= 2 on the unit square.
    B = kc.bound_B(len(X), k, 2.0)
    for r, trace in enumerate(history):
        seq = np.asarray([h[0] for h in trace])
        assert (np.diff(seq) <= B).all(), (name, r, seq)
        assert np.abs(seq - fx["history"][r, :len(seq)]).max() <= len(X) * 2.0 ** -52 * seq.max(), (name, r)
    assert fit.inertia == fit.inertias[fit.best] == min(fit.inertias)


# ---- module -----------------------------------------------------------------------------------------------------
def module_points():
    return cases.init_points()[::3]            # 1000 clustered rows with duplicates, float32


@functools.lru_cache(maxsize=None)
def module_knots():
    """(points, the module, the float64 fits of its levels as fit_balanced_kmeans returned them)."""
    from stnf.models.st_interp import SpatialBasisEmbedding
    pts, fits = module_points(), []
    orig = knot_init.fit_balanced_kmeans
    knot_init.fit_balanced_kmeans = lambda *a, **kw: fits.append(orig(*a, **kw)) or fits[-1]
    try:
        np.random.seed(5)
        emb = SpatialBasisEmbedding(n_centers=[25, 81], init_method='kmeans_balanced', train_coords=pts, init_device=DEV)
    finally:
        knot_init.fit_balanced_kmeans = orig
    return pts, emb, fits


def test_module_with_init_device():
    pts, emb, fits = module_knots()
    assert emb.centers.dtype == torch.float32 and emb.centers.shape == (106, 2) and not emb.centers.is_cuda
    assert emb.bandwidths.dtype == torch.float32 and emb.bandwidths.shape == (106,)
    c = emb.centers.numpy()
    assert np.isfinite(c).all() and c.min() >= 0.0 and c.max() <= 1.0            # means of points of the unit square
    n = len(pts)
    assert len(fits) == 2
    for fit, k, rows in zip(fits, (25, 81), (slice(0, 25), slice(25, 106))):
        # bit for bit the shared helper on the level's float64 centres ...
        fit_c = fit.centers.cpu().numpy()
        assert np.array_equal(c[rows], fit_c.astype(np.float32))
        bw = torch.from_numpy(knot_init.neighbour_bandwidths(fit_c, k, 25)).float().numpy()
        assert np.array_equal(emb.bandwidths.numpy()[rows].view(np.uint32), bw.view(np.uint32))
        assert np.array_equal(bw, kc.knots32(fit_c, k, 25)[1])
        # ... the clusters are within the bounds, and the nearest-centre counts stay sane: every centre is the mean of
        # lo .. hi points, so none is without a nearest point and none is nearest to more than a few clusters' worth
        lo, hi = kc.bounds(n, k)
        cnt = np.bincount(fit.labels.cpu().numpy(), minlength=k)
        near = np.bincount(kc.costs(pts.astype(np.float64), fit_c).argmin(axis=1), minlength=k)
        print(f"k = {k}: bounds {lo}..{hi}, cluster sizes {cnt.min()}..{cnt.max()}, nearest-centre counts "
              f"{near.min()}..{near.max()}, n_iter {fit.n_iter}")
        assert cnt.min() >= lo and cnt.max() <= hi and near.min() >= 1 and near.max() <= 4 * hi


@pytest.mark.parametrize("basis", ["wendland", "triangular"])
def test_forward_on_the_device_equals_the_host_path(basis):
    from stnf.models.st_interp import SpatialBasisEmbedding, _host_phi
    pts, emb0, _ = module_knots()
    emb = SpatialBasisEmbedding(n_centers=[25, 81], basis_function=basis)
    emb.centers.copy_(emb0.centers)
    emb._bandwidths.copy_(emb0.bandwidths)
    coords = torch.from_numpy(np.random.RandomState(3).uniform(0, 1, (301, 2)).astype(np.float32))
    ref = _host_phi(coords.double(), emb.centers.double(), emb.bandwidths.double(), basis).numpy()
    got = emb.to(DEV)(coords.to(DEV)).cpu().numpy()
    assert got.shape == (301, 106)
    assert np.abs(got - ref).max() <= TOL * max(1.0, np.abs(ref).max())


def test_create_model_reads_spatial_init_device():
    from stnf.models import create_model
    pts, emb, _ = module_knots()
    config = dict(k_spatial_centers=[25, 81], k_temporal_centers=[5], hidden_dims=[16],
                  spatial_init_method='kmeans_balanced', spatial_learnable=True, spatial_init_device=DEV)
    np.random.seed(5)
    m = create_model(config, train_coords=pts)
    assert torch.equal(m.spatial_basis.centers.detach(), emb.centers)
    assert torch.equal(m.spatial_basis.bandwidths.detach(), torch.exp(torch.log(emb.bandwidths)))
    with pytest.raises(NotImplementedError):
        create_model(dict(config, spatial_init_device=None), train_coords=pts)
    with pytest.raises(ValueError):
        create_model(dict(config, k_spatial_centers=[25, 4096]), train_coords=pts[:100])
