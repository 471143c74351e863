"""Writes the fixtures of the device-side knot initialiser's tests: tests/golden/gmm_<case>.npz and gmm_achieved.json.

CPU only; needs the real reference on disk and sklearn (like make_golden.py, it runs only in the build container; the
GPU box never runs it and reads only the files):   python tests/golden/make_gmm_golden.py

  gmm_fit_<family>_k<k>.npz   X (n, 2) float64, seeds (3, k) int64 = the k-means++ index arrays of
                              sklearn.cluster.kmeans_plusplus called three times on one RandomState(42), sklearn's
                              weights_, means_, covariances_, lower_bound_, n_iter_ of GaussianMixture(n_components=k,
                              covariance_type='spherical', random_state=42, max_iter=100, n_init=3,
                              init_params='k-means++', reg_covar=1e-6, tol=1e-3).fit(X), and the restatement's
                              (gmm_cases.fit) per-restart n_iter, lower bounds and chosen restart
  gmm_module_sites.npz        coords (12 000, 2) float32, the np.random.seed used, and the centres and bandwidths of the
                              REFERENCE's SpatialBasisEmbedding(n_centers=[25, 81], init_method='gmm') on them
  gmm_achieved.json           "iteration": per one-iteration case and output the largest disagreement of the
                              restatement's 'forward' and 'reversed' chains with its 'pairwise' sums (units of 2^-52, var
                              relative), and the maximum per output; "fit": per fit case the restatement's
                              disagreement D with sklearn (means absolute, variances relative, weights absolute) and
                              the margins of its discrete decisions.
A case that violates a condition of gmm_cases.check_margins is replaced (another seed), never tolerated: this script
fails on it.  The figures are measurements of the restatement against itself and against sklearn, never of the library.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from golden import gmm_cases as gc                       # noqa: E402

N_INIT = 3


def measure_iterations(progress=False):
    """Section "iteration" of gmm_achieved.json (tests/test_gmm_cases_cpu.py re-runs this)."""
    cases_out, worst = {}, {o: 0.0 for o in gc.OUTPUTS}
    for case in gc.ITER_CASES:
        inp = gc.iter_inputs(case)
        ref = gc.em_iteration(inp["X"], inp["w"], inp["mu"], inp["var"], order="pairwise")
        rec = {o: 0.0 for o in gc.OUTPUTS}
        for order in ("forward", "reversed"):
            dis = gc.disagreement(gc.em_iteration(inp["X"], inp["w"], inp["mu"], inp["var"], order=order), ref)
            for o in gc.OUTPUTS:
                rec[o] = max(rec[o], round(dis[o], 3))
        cases_out[case["name"]] = rec
        for o in gc.OUTPUTS:
            worst[o] = max(worst[o], rec[o])
        if progress:
            print(case["name"], rec, flush=True)
    return dict(unit="2^-52 (w, mu, lb absolute; var relative to the reference value)", k_factor=gc.K_FACTOR, max=worst,
                cases=cases_out)


def sklearn_seeds(X, k):
    from sklearn.cluster import kmeans_plusplus
    rs = np.random.RandomState(42)
    return np.stack([kmeans_plusplus(X, k, random_state=rs)[1] for _ in range(N_INIT)]).astype(np.int64)


def sklearn_fit(X, k):
    from sklearn.mixture import GaussianMixture
    return GaussianMixture(n_components=k, covariance_type='spherical', random_state=42, max_iter=gc.MAX_ITER,
                           n_init=N_INIT, init_params='k-means++', reg_covar=gc.REG_COVAR, tol=gc.TOL, verbose=0).fit(X)


def make_fit(case):
    X = gc.fit_points(case)
    k = case["k"]
    seeds = sklearn_seeds(X, k)
    gm = sklearn_fit(X, k)
    res = gc.fit(X, seeds)
    worst, gap = gc.check_margins(res, case["name"])
    assert res["n_iter"][res["best"]] == gm.n_iter_, (case["name"], res["n_iter"], res["best"], gm.n_iter_)
    sk = dict(w=gm.weights_, mu=gm.means_, var=gm.covariances_)
    dis = gc.fit_disagreement(res, sk)
    dis["lb"] = abs(res["lb"] - gm.lower_bound_)
    np.savez_compressed(os.path.join(HERE, f"gmm_{case['name']}.npz"), X=X, seeds=seeds, weights=gm.weights_,
                        means=gm.means_, covariances=gm.covariances_, lower_bound=np.float64(gm.lower_bound_),
                        n_iter=np.int64(gm.n_iter_), re_n_iter=np.asarray(res["n_iter"], np.int64),
                        re_lower_bounds=np.asarray(res["lbs"], np.float64), re_best=np.int64(res["best"]))
    return dict(D=dis, tol_margin=worst, best_gap=gap)


def make_module():
    import torch                                            # noqa: F401
    sys.path.insert(0, "/root/reference")
    from stnf.models.st_interp import SpatialBasisEmbedding as RefEmbedding
    case = gc.MODULE_CASE
    coords = gc.module_coords(case)
    # the conditions hold for what the reference fits as well: the same subsample, the restatement on it
    np.random.seed(case["np_seed"])
    sub = coords[np.random.choice(len(coords), 10000, replace=False)].astype(np.float64)
    margins = {}
    for k in case["n_centers"]:
        res = gc.fit(sub, sklearn_seeds(sub, k))
        margins[str(k)] = gc.check_margins(res, f"{case['name']}_k{k}")
    np.random.seed(case["np_seed"])
    with contextlib.redirect_stdout(io.StringIO()):
        emb = RefEmbedding(n_centers=case["n_centers"], init_method='gmm', train_coords=coords)
    np.savez_compressed(os.path.join(HERE, f"gmm_{case['name']}.npz"), coords=coords, np_seed=np.int64(case["np_seed"]),
                        n_centers=np.asarray(case["n_centers"], np.int64),
                        centers=emb.centers.detach().numpy().astype(np.float32),
                        bandwidths=emb.bandwidths.detach().numpy().astype(np.float32))
    return {k: dict(tol_margin=v[0], best_gap=v[1]) for k, v in margins.items()}


def main():
    table = dict(iteration=measure_iterations(progress="-v" in sys.argv), fit={})
    for case in gc.FIT_CASES:
        table["fit"][case["name"]] = make_fit(case)
        print(case["name"], table["fit"][case["name"]], flush=True)
    table["module"] = make_module()
    with open(gc.ACHIEVED, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", gc.ACHIEVED, "max:", table["iteration"]["max"])


if __name__ == "__main__":
    main()
