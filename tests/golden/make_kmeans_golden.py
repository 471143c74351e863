"""Writes tests/golden/kmeans_fit_*.npz: the whole fits of golden/kmeans_cases.py FIT_CASES by its float64 restatement
(kmeans_cases.fit), with the k-means++ seeds they start from -- sklearn.cluster.kmeans_plusplus on one RandomState(42),
three calls in sequence, what stnf.knot_init.kmeanspp_seeds draws for a level.  Neither the reference nor the library
is imported here.

    python tests/golden/make_kmeans_golden.py

Asserts the conditions of kmeans_cases (MARGIN_TOL, MARGIN_BEST) on every fit it records.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from golden import kmeans_cases as kc  # noqa: E402


def seeds_of(X, k):
    from sklearn.cluster import kmeans_plusplus
    rs = np.random.RandomState(42)
    return np.stack([kmeans_plusplus(X, k, random_state=rs)[1] for _ in range(3)]).astype(np.int64)


def main():
    for case in kc.FIT_CASES:
        X = kc.fit_points(case)
        seeds = seeds_of(X, case["k"])
        res = kc.fit(X, case["k"], list(seeds))
        tol = res["tol"]
        margin = min(abs(s - tol) / tol for s in res["shifts"])
        order = sorted(res["inertias"])
        gap = (order[1] - order[0]) / order[0]
        assert margin >= kc.MARGIN_TOL and gap >= kc.MARGIN_BEST, (case["name"], margin, gap)
        assert all(n < kc.MAX_ITER for n in res["n_iter"]), res["n_iter"]
        hist = np.full((len(seeds), max(res["n_iter"])), np.nan)
        for r, h in enumerate(res["history"]):
            hist[r, :len(h)] = h
        np.savez_compressed(os.path.join(kc.HERE, f"kmeans_{case['name']}.npz"), X=X, seeds=seeds,
                            n_iter=np.asarray(res["n_iter"]), best=np.int64(res["best"]), centers=res["centers"],
                            inertias=np.asarray(res["inertias"]), history=hist, tol=np.float64(tol))
        print(f"{case['name']}: n_iter {res['n_iter']} best {res['best']} inertias {res['inertias']} "
              f"tol margin {margin:.2e} best gap {gap:.2e}")


if __name__ == "__main__":
    main()
