"""Writes tests/golden/seed_*.npz: for every case of golden/seed_cases.py NEW_SKLEARN_CASES the points X, the random
stream (first, u) that seed_cases.draw_stream draws for three restarts of one RandomState(42), and the seed rows that
the installed sklearn.cluster.kmeans_plusplus returns for the same three restarts.  The library is not imported here.

    python tests/golden/make_seed_golden.py

Asserts on every case it records, and on the older gmm_fit_* / kmeans_fit_* fixtures, that the restatement on the
drawn stream gives sklearn's seeds in coordinates: a case on which it does not (a threshold within the rounding of a
prefix sum, or sklearn's expanded distance formula deciding a pick) must get another data seed, not a tolerance.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from golden import seed_cases as sc  # noqa: E402


def sklearn_seeds(X, k):
    import sklearn
    from sklearn.cluster import kmeans_plusplus
    rs = np.random.RandomState(sc.RANDOM_STATE)
    return np.stack([kmeans_plusplus(X, k, random_state=rs)[1] for _ in range(sc.N_INIT)]).astype(np.int64), sklearn.__version__


def main():
    for case in sc.NEW_SKLEARN_CASES:
        X = sc.new_case_points(case)
        seeds, version = sklearn_seeds(X, case["k"])
        first, u = sc.draw_stream(len(X), case["k"], sc.N_INIT)
        rows, pots, _ = sc.restate_runs(X, case["k"], first, u)
        moved = sc.compare_seeds(X, rows, seeds, case["name"])
        np.savez_compressed(os.path.join(sc.HERE, case["name"] + ".npz"), X=X, first=first, u=u, seeds=seeds,
                            sklearn_version=np.asarray(version))
        print(f"{case['name']}: sklearn {version}, {len(np.unique(X, axis=0))} distinct points, {moved} indices name "
              f"another row of the same site, pots {pots}")
    for name in sc.OLD_SKLEARN_FILES:
        fx = sc.sklearn_case(name)
        seeds, _ = sklearn_seeds(fx["X"], fx["seeds"].shape[1])
        assert np.array_equal(seeds, fx["seeds"]), name
        rows, _, _ = sc.restate_runs(fx["X"], seeds.shape[1], fx["first"], fx["u"])
        print(f"{name}: {sc.compare_seeds(fx['X'], rows, seeds, name)} indices name another row of the same site")


if __name__ == "__main__":
    main()
