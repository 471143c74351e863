"""Cases, point generators, float64 restatement and comparator of the tests of the device-side knot initialiser
(stdadk_gmm_em_f64, stnf.knot_init): tests/test_gpu_gmm_init.py, the CPU half in tests/test_gmm_cases_cpu.py, the
fixtures and recorded figures of make_gmm_golden.py.

Numpy only and deterministic (numpy.random.RandomState): the GPU box rebuilds every input of the one-iteration cases;
the fit and module cases come from tests/golden/gmm_*.npz, which also hold what sklearn and the reference computed.

ONE ITERATION (em_iteration): the arithmetic of include/stdadk.h, d = 2, eps = 2^-52 --
    lp_ij = log w_j - 0.5 (d log 2pi + |x_i - mu_j|^2 / var_j) - 0.5 d log var_j      (direct squared distance)
    lpn_i = logsumexp_j lp_ij,  lower_bound = mean_i lpn_i,  r_ij = exp(lp_ij - lpn_i)
    nk_j = sum_i r_ij + 10 eps,  mu'_j = sum_i r_ij x_i / nk_j,
    var'_j = sum_i r_ij |x_i - mu'_j|^2 / (d nk_j) + reg_covar,  w'_j = nk_j / sum_j nk_j
in three orders of summation: 'pairwise' (numpy's pairwise sums over contiguous axes: the reference of the GPU tests),
'forward' (one chain in index order) and 'reversed' (one chain backwards).

THE BOUND of a one-iteration result: per output the largest disagreement between 'pairwise' and the two chains over
all cases below (gmm_achieved.json, section "iteration") times K_FACTOR, the project's factor for what numpy does not
reproduce (fused multiply-adds, the device's exp and log).  w, mu and the lower bound in units of 2^-52 (their scale
is 1: weights sum to 1, the points lie in the unit square, |lpn| is a few units); var relative to the reference value,
in units of 2^-52 as well.  These are measurements of the restatement against itself, never of the library.

WHOLE FIT (fit): GaussianMixture.fit with warm_start=False restated -- per restart the M-step from the one-hot
responsibilities of the seeds, then iterations from lb = -inf until |lb - prev| < tol; the best lower bound wins, the
first on a tie.  The bound of a fit result is K_FACTOR x D, D the restatement's own disagreement with sklearn per case
(gmm_achieved.json, section "fit").  CONDITIONS the generator asserts (check_margins), so that no discrete decision is
within rounding's reach: at every iteration of every restart ||lb - prev| - tol| >= MARGIN_TOL x tol, and the best and
second-best restart lower bounds differ by at least MARGIN_BEST.
"""
import functools
import json
import math
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ACHIEVED = os.path.join(HERE, "gmm_achieved.json")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "st-dadk_amd", "csrc")

EPS = 2.0 ** -52
K_FACTOR = 4.0
D = 2
REG_COVAR = 1e-6
TOL = 1e-3
MAX_ITER = 100
MARGIN_TOL = 1e-3
MARGIN_BEST = 1e-9
OUTPUTS = ("w", "mu", "var", "lb")
FAMILIES = ("uniform", "sites", "clustered")
N_SITES = 500

# the kernels' constants (csrc/gmm.hip), named here so that the shapes below can sit on their edges; kernel_constants()
# reads them back from the source and tests/test_gmm_cases_cpu.py compares
GMM_T = 256               # threads per workgroup = samples per workgroup of the lpn kernel
GMM_KT = 256              # components per LDS tile of the lpn kernel
GMM_MAX_SLABS = 32        # sample slabs per component, at most
GMM_SLAB_FILL = 1024      # slabs = ceil(GMM_SLAB_FILL / k), at most ceil(n / GMM_T)


@functools.lru_cache(maxsize=None)
def kernel_constants():
    src = open(os.path.join(CSRC, "gmm.hip")).read()
    return {name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))
            for name in ("GMM_T", "GMM_KT", "GMM_MAX_SLABS", "GMM_SLAB_FILL")}


def slabs(n, k):
    """csrc/gmm.hip gmm_slabs: (slabs, rows per slab)."""
    s = max(1, min(-(-GMM_SLAB_FILL // k), -(-n // GMM_T), GMM_MAX_SLABS))
    return s, -(-n // s)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31 - 1)


# ------------------------------------------------------------------------------------------------ points
def points(family, n, seed):
    """(n, 2) float64 in the unit square: 'uniform'; 'sites' = N_SITES sites with temporal duplicates (every row is one
    of at most N_SITES distinct coordinates); 'clustered' = eight Gaussian blobs, sigma 0.02 .. 0.08, clipped."""
    rs = np.random.RandomState(seed)
    if family == "uniform":
        return rs.uniform(0.0, 1.0, (n, 2))
    if family == "sites":
        sites = rs.uniform(0.0, 1.0, (N_SITES, 2))
        return sites[rs.randint(0, N_SITES, n)]
    assert family == "clustered", family
    c = rs.uniform(0.15, 0.85, (8, 2))
    sig = rs.uniform(0.02, 0.08, 8)
    j = rs.randint(0, 8, n)
    return np.clip(c[j] + sig[j, None] * rs.standard_normal((n, 2)), 0.0, 1.0)


# ------------------------------------------------------------------------------------------------ one iteration
# (n, k) pairs: the sizes of the issue crossed as a list, then the edges of the kernels' constants -- the sample
# workgroup (n = GMM_T +- 1 is in the list), the component tile (k = GMM_KT -1, +1 likewise, GMM_KT itself added), the
# slab count (ceil(1024 / k) changes between k = 32 | 34, 511 | 512, 1023 | 1024; ceil(n / 256) caps it below
# n = 7 937 for k <= 32; one slab for n <= 256)
ITER_SHAPES = [
    (1, 1), (1, 2), (2, 1), (2, 2), (2, 63), (63, 2), (63, 64), (64, 65), (64, 1), (65, 63), (65, 121), (255, 64),
    (255, 255), (256, 2), (256, 257), (257, 1), (257, 65), (257, 255), (1023, 121), (1023, 1025), (1025, 63),
    (1025, 257), (10000, 1), (10000, 2), (10000, 121), (10000, 255), (10000, 1025),
    (256, 256), (1025, 256), (10000, 32), (10000, 34), (10000, 511), (10000, 512), (10000, 1023), (10000, 1024),
    (7936, 25), (7937, 25), (7937, 33), (513, 2),
]
ITER_CASES = [dict(name=f"iter_{FAMILIES[i % 3]}_n{n}_k{k}", family=FAMILIES[i % 3], n=n, k=k, special=None)
              for i, (n, k) in enumerate(ITER_SHAPES)]
# the three special components, on every family at a shape with several slabs and at a one-workgroup shape
ITER_CASES += [dict(name=f"iter_{fam}_n{n}_k{k}_{sp}", family=fam, n=n, k=k, special=sp)
               for sp in ("massless", "on_point") for fam, n, k in (("sites", 1025, 65), ("uniform", 255, 3),
                                                                      ("clustered", 10000, 121))]
assert len({c["name"] for c in ITER_CASES}) == len(ITER_CASES)
MASSLESS_AT = (50.0, 50.0)        # centre of the component no sample reaches: |x - mu|^2 / (2 var) > 2e9, exp gives 0


def iter_inputs(case):
    """dict(X (n, 2), w (k,), mu (k, 2), var (k,)) float64.  Centres: sample rows (drawn with replacement when n < k)
    moved by N(0, 0.02); variances log-uniform in 1e-4 .. 1e-1 (from 1e-2 with fewer than 8 components, which cannot
    cover the square with narrow ones: |lpn| stays a few units, the scale the lower bound's unit assumes); weights
    positive, summing to 1.  special 'massless': the last component sits at MASSLESS_AT with var = REG_COVAR;
    'on_point': component 0 sits exactly on sample 0 with var = REG_COVAR."""
    n, k = case["n"], case["k"]
    rs = np.random.RandomState(_seed(case["name"]))
    X = points(case["family"], n, _seed(case["name"]) + 1)
    mu = X[rs.randint(0, n, k)] + 0.02 * rs.standard_normal((k, 2))
    var = np.exp(rs.uniform(math.log(1e-4 if k >= 8 else 1e-2), math.log(1e-1), k))
    w = rs.uniform(0.2, 1.0, k)
    w = w / w.sum()
    if case["special"] == "massless":
        mu[k - 1] = MASSLESS_AT
        var[k - 1] = REG_COVAR
    if case["special"] == "on_point":
        mu[0] = X[0]
        var[0] = REG_COVAR
    return dict(X=X, w=w, mu=mu, var=var)


def _sum(a, axis, order):
    """Sum along `axis` of a 2-D array in one of the three orders."""
    a = np.ascontiguousarray(a.T if axis == 0 else a)          # the summed axis last and contiguous
    if order == "pairwise":
        return a.sum(axis=1)
    if a.shape[1] == 0:
        return np.zeros(a.shape[0])
    return np.cumsum(a[:, ::-1] if order == "reversed" else a, axis=1)[:, -1]


def log_prob(X, w, mu, var):
    """lp (n, k)."""
    dx = X[:, 0:1] - mu[None, :, 0]
    dy = X[:, 1:2] - mu[None, :, 1]
    return np.log(w)[None, :] - 0.5 * (D * math.log(2.0 * math.pi) + (dx * dx + dy * dy) / var[None, :]) \
        - 0.5 * D * np.log(var)[None, :]


def em_iteration(X, w, mu, var, reg_covar=REG_COVAR, order="pairwise", mutate=None):
    """One EM iteration in float64 numpy: dict(w, mu, var, lb).  `mutate` states a wrong iteration for
    tests/test_gmm_cases_cpu.py: 'old_mean' (variance about the old mean), 'drop_sample' (the last sample left out of
    the M-step's sums)."""
    X, w, mu, var = (np.asarray(a, np.float64) for a in (X, w, mu, var))
    n = X.shape[0]
    lp = log_prob(X, w, mu, var)
    m = lp.max(axis=1)
    lpn = m + np.log(_sum(np.exp(lp - m[:, None]), 1, order))
    lb = float(_sum(lpn[None, :], 1, order)[0] / n)
    r = np.exp(lp - lpn[:, None])
    if mutate == "drop_sample":
        r, X = r[:-1], X[:-1]
    nk = _sum(r, 0, order) + 10.0 * EPS
    mu_new = np.stack([_sum(r * X[:, 0:1], 0, order), _sum(r * X[:, 1:2], 0, order)], axis=1) / nk[:, None]
    about = mu if mutate == "old_mean" else mu_new
    ex = X[:, 0:1] - about[None, :, 0]
    ey = X[:, 1:2] - about[None, :, 1]
    var_new = _sum(r * (ex * ex + ey * ey), 0, order) / (D * nk) + reg_covar
    return dict(w=nk / _sum(nk[None, :], 1, order)[0], mu=mu_new, var=var_new, lb=lb)


def disagreement(got, ref):
    """{output: the largest disagreement in units of 2^-52} -- absolute for w, mu, lb, relative to ref for var."""
    return dict(w=float(np.abs(np.asarray(got["w"]) - ref["w"]).max() / EPS),
                mu=float(np.abs(np.asarray(got["mu"]) - ref["mu"]).max() / EPS),
                var=float((np.abs(np.asarray(got["var"]) - ref["var"]) / ref["var"]).max() / EPS),
                lb=float(abs(float(got["lb"]) - ref["lb"]) / EPS))


@functools.lru_cache(maxsize=None)
def achieved():
    return json.load(open(ACHIEVED))


def bounds():
    """{output: bound in units of 2^-52} of the GPU tests: K_FACTOR x the recorded maximum over the cases."""
    return {o: K_FACTOR * float(achieved()["iteration"]["max"][o]) for o in OUTPUTS}


def compare_iteration(got, ref, name, K=None):
    """One result (dict w, mu, var, lb; arrays of the reference's shapes) against em_iteration(order='pairwise').
    Asserts shapes, that every value is finite, and the bound per output; returns the disagreement for printing."""
    K = bounds() if K is None else K
    for o in ("w", "mu", "var"):
        g = np.asarray(got[o])
        assert g.shape == ref[o].shape and g.dtype == np.float64, (name, o, g.shape, g.dtype)
        assert np.isfinite(g).all(), (name, o, "not finite")
    assert math.isfinite(float(got["lb"])), (name, "lb not finite")
    dis = disagreement(got, ref)
    for o in OUTPUTS:
        assert dis[o] <= K[o], (name, o, dis[o], "bound", K[o])
    return dis


def fmt(dis):
    return ", ".join(f"{o} {dis[o]:.2f}" for o in OUTPUTS)


# ------------------------------------------------------------------------------------------------ whole fit
FIT_N = 4000
FIT_CASES = [dict(name=f"fit_{fam}_k{k}", family=fam, k=k, n=FIT_N) for fam in FAMILIES for k in (25, 81)]
MODULE_CASE = dict(name="module_sites", n_centers=[25, 81], rows=12000, np_seed=20240611)


def fit_points(case):
    return points(case["family"], case["n"], _seed(case["name"]))


def module_coords(case=MODULE_CASE):
    """(rows, 2) float32 training coordinates: 500 sites with temporal duplicates, more rows than the subsample takes."""
    return points("sites", case["rows"], _seed(case["name"])).astype(np.float32)


def seed_parameters(X, idx, reg_covar=REG_COVAR):
    """The M-step from one-hot responsibilities on the seed rows."""
    x = np.asarray(X, np.float64)[np.asarray(idx, np.int64)]
    nk = 1.0 + 10.0 * EPS
    mu = x / nk
    return np.full(len(x), nk / len(X)), mu, ((x - mu) ** 2).sum(axis=1) / (D * nk) + reg_covar


def fit(X, seed_indices, max_iter=MAX_ITER, tol=TOL, reg_covar=REG_COVAR, order="pairwise"):
    """The whole fit in float64 numpy: dict(w, mu, var, lb, n_iter [per restart], lbs [per restart], best,
    trace [per restart the lower bound of every iteration])."""
    best, out, n_iter, lbs, trace = -1, None, [], [], []
    for r, idx in enumerate(seed_indices):
        w, mu, var = seed_parameters(X, idx, reg_covar)
        lb, it, tr = -math.inf, 0, []
        for it in range(1, max_iter + 1):
            prev = lb
            res = em_iteration(X, w, mu, var, reg_covar, order)
            w, mu, var, lb = res["w"], res["mu"], res["var"], res["lb"]
            tr.append(lb)
            if abs(lb - prev) < tol:
                break
        n_iter.append(it)
        lbs.append(lb)
        trace.append(tr)
        if best < 0 or lb > lbs[best]:
            best, out = r, (w, mu, var)
    return dict(w=out[0], mu=out[1], var=out[2], lb=lbs[best], n_iter=n_iter, lbs=lbs, best=best, trace=trace)


def check_margins(res, name, tol=TOL):
    """The conditions of the module docstring on a fit() result; returns (smallest ||dlb| - tol| / tol, gap between the
    two best restarts)."""
    worst = math.inf
    for tr in res["trace"]:
        prev = -math.inf
        for lb in tr:
            worst = min(worst, abs(abs(lb - prev) - tol) / tol)
            prev = lb
    top = sorted(res["lbs"], reverse=True)
    gap = top[0] - top[1] if len(top) > 1 else math.inf
    assert worst >= MARGIN_TOL, (name, "an iteration's |dlb| is within", worst, "of tol")
    assert gap >= MARGIN_BEST, (name, "best and second-best restart differ by", gap)
    return worst, gap


def fit_disagreement(got, ref):
    """dict(mu, var, w): |means| absolute, variances relative to ref, weights absolute."""
    return dict(mu=float(np.abs(np.asarray(got["mu"]) - ref["mu"]).max()),
                var=float((np.abs(np.asarray(got["var"]) - ref["var"]) / ref["var"]).max()),
                w=float(np.abs(np.asarray(got["w"]) - ref["w"]).max()))


def grid_bandwidth(k):
    side = int(math.sqrt(k))
    return 2.5 * (1.0 / (side - 1) if side > 1 else 1.0)


def knots32(mu, var, k):
    """The reference's rule on a level's float64 fit: (centres, bandwidths) float32."""
    bw = np.clip(4.23 * 2.5 * np.sqrt(np.asarray(var, np.float64)), 0.25 * grid_bandwidth(k), float("inf"))
    return np.asarray(mu, np.float64).astype(np.float32), bw.astype(np.float32)


def ulps32(got, ref):
    """Largest distance in float32 units in the last place (of the reference's magnitude)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    return float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)).max())
