"""The CPU half of the device-side knot initialiser's tests (tests/test_gpu_gmm_init.py), no GPU needed:
  * the float64 restatement (golden/gmm_cases.py) reproduces the committed sklearn fits (golden/gmm_fit_*.npz): per-restart
    n_iter and the chosen restart equal, the values within the recorded D, and the conditions on its discrete decisions;
  * re-measuring the summation-order disagreement reproduces golden/gmm_achieved.json;
  * the comparator, at the GPU tests' own bounds, rejects a variance taken about the old mean and a dropped sample;
  * the constants gmm_cases names are the kernels'; stnf.knot_init's host-side pieces equal the restatement's;
  * the argument checks of stdadk_gmm_em_f64, in a child process under STDADK_DRY_RUN=1 (validates, launches nothing)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden import gmm_cases as gc
from golden import make_gmm_golden as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [c["name"] for c in gc.FIT_CASES])
def test_restatement_reproduces_the_sklearn_golden(name):
    fx = np.load(os.path.join(gc.HERE, f"gmm_{name}.npz"))
    res = gc.fit(fx["X"], list(fx["seeds"]))
    assert res["n_iter"] == fx["re_n_iter"].tolist() and res["best"] == int(fx["re_best"])
    assert res["n_iter"][res["best"]] == int(fx["n_iter"])
    assert np.abs(np.asarray(res["lbs"]) - fx["re_lower_bounds"]).max() <= 1e-12
    gc.check_margins(res, name)
    rec = gc.achieved()["fit"][name]
    dis = gc.fit_disagreement(res, dict(w=fx["weights"], mu=fx["means"], var=fx["covariances"]))
    for o in ("mu", "var", "w"):
        assert dis[o] <= rec["D"][o], (name, o, dis[o], rec["D"][o])
    assert abs(res["lb"] - float(fx["lower_bound"])) <= rec["D"]["lb"]
    # the seeds are rows of X, one per component, and the fixture's points are the generator's
    assert fx["seeds"].shape == (3, int(name.rsplit("k", 1)[1])) and fx["seeds"].max() < len(fx["X"])
    assert np.array_equal(fx["X"], gc.fit_points(next(c for c in gc.FIT_CASES if c["name"] == name)))


def test_module_fixture_holds_the_generators_coordinates():
    fx = np.load(os.path.join(gc.HERE, f"gmm_{gc.MODULE_CASE['name']}.npz"))
    assert np.array_equal(fx["coords"], gc.module_coords()) and fx["coords"].dtype == np.float32
    assert int(fx["np_seed"]) == gc.MODULE_CASE["np_seed"] and fx["n_centers"].tolist() == gc.MODULE_CASE["n_centers"]
    assert fx["centers"].shape == (106, 2) and fx["bandwidths"].shape == (106,)
    assert fx["centers"].dtype == np.float32 and fx["bandwidths"].dtype == np.float32
    for k, rec in gc.achieved()["module"].items():
        assert rec["tol_margin"] >= gc.MARGIN_TOL and rec["best_gap"] >= gc.MARGIN_BEST, (k, rec)


def test_recorded_iteration_figures_are_reproduced():
    """Regenerating the "iteration" section changes nothing beyond what another CPU's exp and log may move (a quarter
    of the recorded maximum); every case has a record; the bound the GPU tests use follows from it."""
    table = gc.achieved()["iteration"]
    fresh = mg.measure_iterations()
    assert set(table["cases"]) == {c["name"] for c in gc.ITER_CASES} == set(fresh["cases"])
    assert table["k_factor"] == gc.K_FACTOR
    for o in gc.OUTPUTS:
        assert 0.75 * table["max"][o] <= fresh["max"][o] <= 1.25 * table["max"][o], (o, fresh["max"][o], table["max"][o])
        assert gc.bounds()[o] == gc.K_FACTOR * table["max"][o]


@pytest.mark.parametrize("name", ["iter_sites_n1025_k65_on_point", "iter_clustered_n10000_k121_massless"])
def test_comparator_has_teeth(name):
    case = next(c for c in gc.ITER_CASES if c["name"] == name)
    inp = gc.iter_inputs(case)
    ref = gc.em_iteration(inp["X"], inp["w"], inp["mu"], inp["var"])
    gc.compare_iteration(gc.em_iteration(inp["X"], inp["w"], inp["mu"], inp["var"], order="forward"), ref, name)
    for mutate in ("old_mean", "drop_sample"):
        bad = gc.em_iteration(inp["X"], inp["w"], inp["mu"], inp["var"], mutate=mutate)
        with pytest.raises(AssertionError):
            gc.compare_iteration(bad, ref, name)
    nan = dict(ref, var=np.where(np.arange(case["k"]) == 1, np.nan, ref["var"]))
    with pytest.raises(AssertionError):
        gc.compare_iteration(nan, ref, name)


def test_special_components_of_the_reference():
    """The massless component: no responsibility at all, so mu' = 0 and var' = reg_covar exactly, in the restatement."""
    for case in gc.ITER_CASES:
        if case["special"] != "massless":
            continue
        inp = gc.iter_inputs(case)
        ref = gc.em_iteration(inp["X"], inp["w"], inp["mu"], inp["var"])
        j = case["k"] - 1
        assert np.all(ref["mu"][j] == 0.0) and ref["var"][j] == gc.REG_COVAR and 0.0 < ref["w"][j] < 1e-15


def test_named_constants_are_the_kernels():
    assert gc.kernel_constants() == dict(GMM_T=gc.GMM_T, GMM_KT=gc.GMM_KT, GMM_MAX_SLABS=gc.GMM_MAX_SLABS,
                                         GMM_SLAB_FILL=gc.GMM_SLAB_FILL)
    from stnf import _native as N
    for n, k in gc.ITER_SHAPES:
        assert N.gmm_workspace_bytes(n, k) == 8 * (n + -(-n // gc.GMM_T) + 4 * k * gc.slabs(n, k)[0]), (n, k)


def test_host_side_pieces_of_knot_init_equal_the_restatement():
    from stnf import knot_init
    X = gc.points("sites", 300, 5)
    idx = np.random.RandomState(1).choice(300, 25, replace=False)
    for a, b in zip(knot_init.seed_parameters(X, idx, gc.REG_COVAR), gc.seed_parameters(X, idx)):
        assert np.array_equal(a, b)
    var = np.exp(np.random.RandomState(2).uniform(np.log(1e-6), np.log(1e-1), 25))
    c, b = knot_init.knots_from_fit(X[:25], var, 25)
    c_ref, b_ref = gc.knots32(X[:25], var, 25)
    assert np.array_equal(c.numpy(), c_ref) and np.array_equal(b.numpy(), b_ref)
    assert (b_ref == np.float32(0.25 * 2.5 / 4)).any() and (b_ref > 0.25 * 2.5 / 4).any()      # both sides of the floor


def test_init_device_plumbing_without_a_gpu():
    from stnf.models.st_interp import STInterpMLP, SpatialBasisEmbedding
    coords = gc.points("uniform", 64, 3).astype(np.float32)
    with pytest.raises(RuntimeError, match="HIP device"):
        SpatialBasisEmbedding(n_centers=[4], init_method='gmm', train_coords=coords, init_device='cpu')
    a = SpatialBasisEmbedding(n_centers=[9], init_device='cuda')                   # every other initialiser ignores it
    assert torch.equal(a.centers, SpatialBasisEmbedding(n_centers=[9]).centers)
    m = STInterpMLP(k_spatial_centers=[9], k_temporal_centers=[5], hidden_dims=[16], spatial_init_device='cuda')
    assert torch.equal(m.spatial_basis.centers, a.centers)


# ---- the entry's argument checks ----------------------------------------------------------------------------------
def drive():
    """Child process under STDADK_DRY_RUN=1: messages of the entry's argument checks."""
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    from stnf import _native as N
    n, k = 1000, 121
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)                            # noqa: E731
    need = N.gmm_workspace_bytes(n, k)
    rec = {"need": need}

    def call(key, n=n, k=k, reg=1e-6, short=0, alias=None):
        a = dict(X=z(n, 2), w=z(k), mu=z(k, 2), var=z(k), w_out=z(k), mu_out=z(k, 2), var_out=z(k), lb=z(1))
        ws = z(max(N.lib().stdadk_gmm_workspace_bytes(max(n, 1), min(max(k, 1), 65536)) // 8 - short, 1))
        if alias == "w":
            a["w_out"] = a["w"]
        if alias == "mu_in_ws":
            a["mu_out"] = ws[:2 * k].view(k, 2)
        if alias == "var_mu":
            a["var_out"] = a["mu"].view(-1)[k:]
        try:
            N.gmm_em(a["X"], a["w"], a["mu"], a["var"], reg, a["w_out"], a["mu_out"], a["var_out"], a["lb"], ws)
            rec[key] = None
        except RuntimeError as e:
            rec[key] = str(e)
    call("good")
    call("good_small", n=1, k=1)
    call("n0", n=0)
    call("k0", k=0)
    call("k_big", k=65537)
    call("reg0", reg=0.0)
    call("reg_nan", reg=float("nan"))
    call("alias_w", alias="w")
    call("alias_ws", alias="mu_in_ws")
    call("alias_overlap", alias="var_mu")
    call("workspace", short=1)
    for key, args in (("ws_n0", (0, 5)), ("ws_n_big", (1 << 31, 5)), ("ws_k0", (5, 0)), ("ws_k_big", (5, 65537))):
        try:
            N.gmm_workspace_bytes(*args)
            rec[key] = None
        except RuntimeError as e:
            rec[key] = str(e)
    print("RECORD " + json.dumps(rec))


@pytest.fixture(scope="module")
def rec():
    env = dict(os.environ, STDADK_DRY_RUN="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RECORD ")][-1]
    return json.loads(line[len("RECORD "):])


def test_entry_accepts_good_arguments(rec):
    assert rec["good"] is None and rec["good_small"] is None
    assert rec["need"] == 8 * (1000 + 4 + 121 * 4 * 4)            # lpn, 4 sample workgroups, 4 slabs x 4 values per component


@pytest.mark.parametrize("case,word", [("n0", "n=0"), ("k0", "k=0"), ("k_big", "k=65537"), ("reg0", "reg_covar"),
                                       ("reg_nan", "reg_covar"), ("alias_w", "alias"), ("alias_ws", "alias"),
                                       ("alias_overlap", "alias"), ("workspace", "workspace"), ("ws_n0", "bad sizes"),
                                       ("ws_n_big", "bad sizes"), ("ws_k0", "bad sizes"), ("ws_k_big", "bad sizes")])
def test_entry_refuses_bad_arguments(rec, case, word):
    assert rec[case] is not None and word in rec[case], rec[case]


if __name__ == "__main__":
    drive()
