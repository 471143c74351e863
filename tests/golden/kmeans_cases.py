"""Cases, float64 restatement, oracle and comparator of the tests of the balanced k-means knot initialiser
(stdadk_kmeans_balanced_iter_f64, stnf.knot_init.fit_balanced_kmeans): tests/test_gpu_kmeans_balanced.py, the CPU half
in tests/test_kmeans_cases_cpu.py, the fixtures of make_kmeans_golden.py.  Numpy and scipy only, deterministic.

THE CONTRACT (include/stdadk.h).  Bounds of a level of k knots on n points: lo = max(1, n // k - 1), hi = n // k + n % k.
One iteration on centres mu:
    c_ij   = (x_i - mu_jx)^2 + (y_i - mu_jy)^2, every operation rounded once (no fused multiply-add);
    q_ij   = rint(c_ij 2^s), s = 52 - e with max c = f 2^e, 0.5 <= f < 1 (s = 0 when max c = 0): the costs on ONE
             binary grid of spacing 2^-s <= max c 2^-51, as 64-bit integers, so that every path sum below is exact and
             a cycle of exact weight 0 (duplicated points produce them) can never round to a negative one;
    E-step : labels minimising sum_i q[i][labels[i]] subject to lo <= |cluster j| <= hi -- the EXACT optimum, by
             successive shortest paths from the nearest-centre assignment (e_step below states it move for move);
    inertia = sum_i c[i][labels[i]];  M-step: mu'_j = mean of the members of j;  shift = sum |mu' - mu|^2.
An assignment optimal for q is within 2 n 2^-s / 2 <= n max c 2^-51 of the optimum for c, far inside the bound
    B = 16 (n + k) 2^-53 n max c
of the tests (each c within 4 ulp; an assignment optimal for perturbed costs is off by at most twice the summed
perturbation of n terms; a path sum adds at most k + 1 roundings).

THE ORACLE (oracle): scipy.optimize.linear_sum_assignment on the float64 costs c -- k hi slot columns, the first
lo of each cluster mandatory; rows = the n points, then k hi - n dummies; a point costs c_ij on every slot of j, a dummy
0 on an optional slot and 1e6 on a mandatory one.  Costs are compared, never labels: the optimum need not be unique.
"""
import functools
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "st-dadk_amd", "csrc")

INF = np.int64(1) << np.int64(62)
MAX_ITER = 100
TOL_FACTOR = 1e-4
N_SITES = 40

# the kernels' constants (csrc/kmeans.hip), named here so that the shapes below can sit on their edges;
# kernel_constants() reads them back from the source and tests/test_kmeans_cases_cpu.py compares
KM_T = 256                # threads and points per workgroup of the cost kernels; threads of the M-step workgroups
KM_KT = 256               # centres per LDS tile of the cost kernels
KM_AT = 1024              # threads of the one workgroup that balances the assignment
KM_MAX_K = 1023           # k + 1 nodes (the clusters and the sink) fit the balancing workgroup


@functools.lru_cache(maxsize=None)
def kernel_constants():
    src = open(os.path.join(CSRC, "kmeans.hip")).read()
    return {name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))
            for name in ("KM_T", "KM_KT", "KM_AT", "KM_MAX_K")}


def bounds(n, k):
    """(lo, hi) of the reference (stnf/models/st_interp.py:379-385)."""
    if k > n:
        raise ValueError(f"kmeans_balanced: {k} knots on {n} points")
    return max(1, n // k - 1), n // k + n % k


def bound_B(n, k, max_c):
    return 16.0 * (n + k) * 2.0 ** -53 * n * max_c


# ------------------------------------------------------------------------------------------------ points and cases
def points(family, n, seed, n_sites=N_SITES):
    """(n, 2) float64 in the unit square: 'uniform'; 'sites' = n_sites sites x times (every row one of n_sites distinct
    coordinates); 'clustered' = five Gaussian blobs; 'identical' = one coordinate n times."""
    rs = np.random.RandomState(seed)
    if family == "uniform":
        return rs.uniform(0.0, 1.0, (n, 2))
    if family == "sites":
        sites = rs.uniform(0.0, 1.0, (n_sites, 2))
        return sites[rs.randint(0, n_sites, n)]
    if family == "identical":
        return np.tile(rs.uniform(0.2, 0.8, (1, 2)), (n, 1))
    assert family == "clustered", family
    c = rs.uniform(0.15, 0.85, (5, 2))
    sig = rs.uniform(0.02, 0.08, 5)
    j = rs.randint(0, 5, n)
    return np.clip(c[j] + sig[j, None] * rs.standard_normal((n, 2)), 0.0, 1.0)


# (family, n, k, special): every k hi <= 2000.  special 'far' moves the last centre to (5, 5): no point is nearest to
# it and it must be filled to lo, 'far8' does so with the last eight; 'spread' takes the centres uniform in the square and
# not from the points.
_SHAPES = [
    ("clustered", 60, 6, None),            # n % k == 0: hi = n / k, so every cluster holds exactly n / k
    ("uniform", 48, 48, "spread"), ("uniform", 20, 20, None),            # k = n
    ("sites", 1, 1, None), ("clustered", 50, 1, None),                   # k = 1
    ("clustered", 97, 9, None),            # n % k != 0, both bounds binding on clustered points
    ("clustered", 130, 25, "far"), ("uniform", 61, 7, "far"),            # a centre no point is nearest to
    ("sites", 240, 12, None), ("sites", 200, 40, "spread"),              # sites x times duplicates (40 sites, 40 centres)
    ("identical", 33, 4, None), ("identical", 12, 12, None),             # all points identical
    ("uniform", 2, 2, None), ("uniform", 3, 2, None), ("clustered", 64, 2, None),
    # the edges of KM_T (points per workgroup) and of KM_AT (the balancing workgroup's stride)
    ("clustered", 255, 7, None), ("uniform", 256, 7, None), ("sites", 257, 7, None),
    ("uniform", 1023, 4, None), ("clustered", 1024, 4, None), ("clustered", 1025, 4, None),
    # the edges of KM_KT (centre tile) and of the row layout of the balancing workgroup, which changes at every power
    # of two of k (k = 2^m | 2^m + 1) up to KM_AT / 2, and the largest k
    ("uniform", 256, 255, "spread"), ("uniform", 257, 256, "spread"), ("clustered", 258, 257, "spread"),
    ("uniform", 70, 32, "spread"), ("uniform", 70, 33, "spread"), ("uniform", 513, 512, "spread"),
    ("uniform", 514, 513, "spread"), ("uniform", 1023, 1023, "far8"),
]
CASES = [dict(name=f"{fam}_n{n}_k{k}" + (f"_{sp}" if sp else ""), family=fam, n=n, k=k, special=sp)
         for fam, n, k, sp in _SHAPES]
assert all(bounds(c["n"], c["k"])[1] * c["k"] <= 2000 for c in CASES)
assert len({c["name"] for c in CASES}) == len(CASES)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31 - 1)


def case_inputs(case):
    """dict(X (n, 2), mu (k, 2), lo, hi) of a one-iteration case."""
    n, k = case["n"], case["k"]
    X = points(case["family"], n, _seed(case["name"]))
    rs = np.random.RandomState(_seed(case["name"]) + 1)
    mu = X[rs.choice(n, k, replace=False)].copy()
    if case["special"] == "spread":
        mu = rs.uniform(0.0, 1.0, (k, 2))
    if case["special"] == "far":
        mu[-1] = (5.0, 5.0)
    if case["special"] == "far8":
        mu[-8:] = 5.0 + 0.25 * np.arange(16.0).reshape(8, 2)
    lo, hi = bounds(n, k)
    return dict(X=X, mu=mu, lo=lo, hi=hi)


# whole fits (tests/golden/kmeans_fit_*.npz, written by make_kmeans_golden.py from fit() below): n = 1200, k in {9, 25}
FIT_N = 1200
FIT_SITES = 150
FIT_CASES = [dict(name=f"fit_{fam}_k{k}", family=fam, k=k) for fam in ("clustered", "sites", "uniform") for k in (9, 25)]
# conditions the generator asserts, so that no discrete decision of a fit is within rounding's reach: at every
# iteration |shift - tol| >= MARGIN_TOL x tol, and the two lowest restart inertias differ by MARGIN_BEST (relative)
MARGIN_TOL = 1e-6
MARGIN_BEST = 1e-9
CENTRE_TOL = 1e-9


def fit_points(case):
    return points(case["family"], FIT_N, _seed(case["name"]), n_sites=FIT_SITES)


# ------------------------------------------------------------------------------------------------ one iteration
def costs(X, mu):
    dx = X[:, None, 0] - mu[None, :, 0]
    dy = X[:, None, 1] - mu[None, :, 1]
    return dx * dx + dy * dy


def quantise(c):
    m = float(c.max())
    s = 0 if m <= 0.0 else 52 - int(np.frexp(m)[1])
    return np.rint(np.ldexp(c, s)).astype(np.int64)


def _row(q, labels, a):
    """w(a -> b) = min over the members i of a of q[i][b] - q[i][a], the lowest such i; INF for an empty cluster."""
    k = q.shape[1]
    idx = np.flatnonzero(labels == a)
    if len(idx) == 0:
        return np.full(k, INF), np.full(k, -1, np.int64)
    d = q[idx] - q[idx, a][:, None]
    j = d.argmin(axis=0)
    w = d[j, np.arange(k)]
    w[a] = INF
    return w, idx[j]


def e_step(q, lo, hi, stats=None):
    """The exact constrained assignment for the integer costs q (n, k): labels.  Nodes 0 .. k-1 are the clusters, k is
    the sink T.  Bellman-Ford runs in synchronous rounds (every node reads the distances of the round before), the
    lowest predecessor index wins a tie, a distance moves only when it gets strictly smaller (so only the nodes that
    moved in the round before are read as predecessors: the others were candidates already)."""
    n, k = q.shape
    T = k
    labels = q.argmin(axis=1)
    cnt = np.bincount(labels, minlength=k).astype(np.int64)
    f = np.clip(cnt, lo, hi)
    imb = np.concatenate([cnt - f, [f.sum() - n]])
    W = np.full((k + 1, k + 1), INF)
    arg = np.full((k, k), -1, np.int64)
    for a in range(k):
        W[a, :k], arg[a] = _row(q, labels, a)
    n_aug = 0
    while (imb > 0).any():
        n_aug += 1
        assert n_aug <= n, "more augmentations than points"
        W[:k, T] = np.where(f < hi, 0, INF)
        W[T, :k] = np.where(f > lo, 0, INF)
        dist = np.where(imb > 0, np.int64(0), INF)
        pred = np.full(k + 1, -1, np.int64)
        front = np.flatnonzero(imb > 0)                 # only a node whose distance moved last round can improve one
        for rnd in range(k + 2):
            Wf = W[front]
            cand = np.where(Wf < INF, dist[front, None] + np.where(Wf < INF, Wf, 0), INF)
            j = cand.argmin(axis=0)                     # the first minimum: the lowest predecessor index
            best = cand[j, np.arange(k + 1)]
            upd = best < dist
            if not upd.any():
                break
            dist = np.where(upd, best, dist)
            pred = np.where(upd, front[j], pred)
            front = np.flatnonzero(upd)
        else:
            raise AssertionError("Bellman-Ford did not settle in k + 2 rounds: a negative cycle")
        sinks = np.flatnonzero((imb < 0) & (dist < INF))
        assert len(sinks), "no deficit node reachable"
        v = sinks[dist[sinks].argmin()]
        imb[v] += 1
        path = [v]
        while pred[path[-1]] >= 0:
            path.append(pred[path[-1]])
            assert len(path) <= k + 1, "predecessors form a cycle"
        path.reverse()
        imb[path[0]] -= 1
        changed = []
        for a, b in zip(path[:-1], path[1:]):
            if b == T:
                f[a] += 1
            elif a == T:
                f[b] -= 1
            else:
                labels[arg[a, b]] = b
                changed += [a, b]
        for a in dict.fromkeys(changed):
            W[a, :k], arg[a] = _row(q, labels, a)
    if stats is not None:
        stats["augmentations"] = n_aug
    return labels


def m_step(X, labels, k):
    mu = np.empty((k, 2))
    for j in range(k):
        mu[j] = X[labels == j].mean(axis=0)
    return mu


def iteration(X, mu, lo, hi, stats=None):
    """dict(labels, mu (the new centres), inertia, shift) of one iteration on centres mu."""
    c = costs(X, mu)
    labels = e_step(quantise(c), lo, hi, stats)
    new = m_step(X, labels, mu.shape[0])
    return dict(labels=labels, mu=new, inertia=float(c[np.arange(len(X)), labels].sum()),
                shift=float(((new - mu) ** 2).sum()))


def fit(P, k, seeds, max_iter=MAX_ITER, tol_factor=TOL_FACTOR):
    """The whole fit: dict(centers, labels, inertia, n_iter [per restart], best, inertias [per restart], history [per
    restart the inertia of every iteration]).  The lowest inertia wins, the first restart on a tie."""
    n = len(P)
    lo, hi = bounds(n, k)
    tol = tol_factor * float(np.mean(np.var(P, axis=0)))
    out = dict(n_iter=[], inertias=[], history=[], shifts=[], best=-1, tol=tol)
    for r, idx in enumerate(seeds):
        mu = P[np.asarray(idx, np.int64)].copy()
        hist = []
        for it in range(1, max_iter + 1):
            res = iteration(P, mu, lo, hi)
            mu = res["mu"]
            hist.append(res["inertia"])
            out["shifts"].append(res["shift"])
            if res["shift"] <= tol:
                break
        out["n_iter"].append(it)
        out["inertias"].append(res["inertia"])
        out["history"].append(hist)
        if out["best"] < 0 or res["inertia"] < out["inertia"]:
            out.update(best=r, inertia=res["inertia"], centers=mu, labels=res["labels"])
    return out


def knots32(centers64, k, k0):
    """(centres, bandwidths) float32 of a level: bandwidth = 2.5 x the mean distance to the min(4, k - 1) nearest
    other centres (scipy cdist on the float64 centres), the grid bandwidth of k0 = n_centers[0] knots for k == 1."""
    from scipy.spatial.distance import cdist
    c = np.asarray(centers64, np.float64)
    dist = cdist(c, c)
    np.fill_diagonal(dist, np.inf)
    nn = min(4, k - 1) if k > 1 else 1
    bw = 2.5 * np.sort(dist, axis=1)[:, :nn].mean(axis=1)
    if k == 1:
        side = int(np.sqrt(k0))
        bw = np.array([2.5 * (1.0 / (side - 1) if side > 1 else 1.0)])
    return c.astype(np.float32), bw.astype(np.float32)


# ------------------------------------------------------------------------------------------------ oracle, comparator
def oracle(c, lo, hi):
    """(optimal cost, one optimal labelling) of the constrained assignment on the float64 costs c, by
    scipy.optimize.linear_sum_assignment."""
    from scipy.optimize import linear_sum_assignment
    n, k = c.shape
    m = k * hi
    cost = np.empty((m, m))
    cost[:n] = np.repeat(c, hi, axis=1)
    mandatory = (np.arange(m) % hi) < lo
    cost[n:] = np.where(mandatory, 1e6, 0.0)[None, :]
    rows, cols = linear_sum_assignment(cost)
    labels = np.empty(n, np.int64)
    labels[rows[rows < n]] = cols[rows < n] // hi
    assert cost[rows[rows >= n], cols[rows >= n]].sum() == 0.0, "a mandatory slot went to a dummy"
    return float(c[np.arange(n), labels].sum()), labels


def assignment_cost(c, labels):
    return float(c[np.arange(c.shape[0]), np.asarray(labels, np.int64)].sum())


def compare_assignment(labels, c, lo, hi, optimum, what):
    """labels in range, every count within [lo, hi] exactly, and the float64 cost of the labels within B of the
    optimum (on either side: below it would mean a broken oracle)."""
    n, k = c.shape
    labels = np.asarray(labels)
    assert labels.shape == (n,) and labels.min() >= 0 and labels.max() < k, f"{what}: labels out of range"
    cnt = np.bincount(labels, minlength=k)
    assert cnt.min() >= lo and cnt.max() <= hi, f"{what}: counts {cnt.min()}..{cnt.max()} outside [{lo}, {hi}]"
    B = bound_B(n, k, float(c.max()))
    gap = assignment_cost(c, labels) - optimum
    assert abs(gap) <= B, f"{what}: cost gap {gap:.3e} beyond B = {B:.3e}"
    return gap


# ---- wrong answers the comparator must refuse ---------------------------------------------------------------------
def worst_swap(c, labels):
    """The optimum with the two points of different clusters exchanged that raises the cost most (feasible: the
    counts stay); None when no exchange raises it (k == 1, or every cost equal)."""
    n = c.shape[0]
    own = c[np.arange(n), labels]
    to = c[:, labels]                                  # to[i][i2] = cost of i in the cluster of i2
    delta = to + to.T - own[:, None] - own[None, :]
    delta[labels[:, None] == labels[None, :]] = -np.inf
    i, i2 = np.unravel_index(delta.argmax(), delta.shape)
    if not delta[i, i2] > 0:
        return None
    out = labels.copy()
    out[i], out[i2] = labels[i2], labels[i]
    return out


def greedy_repair(c, lo, hi):
    """Nearest centre, then one point at a time: while a cluster is over hi its cheapest-to-move member goes to the
    cheapest cluster under hi; while one is under lo it takes the cheapest point of a cluster above lo."""
    n, k = c.shape
    labels = c.argmin(axis=1)
    cnt = np.bincount(labels, minlength=k)
    while (cnt > hi).any():
        a = int(np.flatnonzero(cnt > hi)[0])
        idx = np.flatnonzero(labels == a)
        d = np.where((cnt < hi)[None, :], c[idx] - c[idx, a][:, None], np.inf)
        i, b = np.unravel_index(d.argmin(), d.shape)
        labels[idx[i]] = b
        cnt[a] -= 1
        cnt[b] += 1
    while (cnt < lo).any():
        b = int(np.flatnonzero(cnt < lo)[0])
        d = np.where(cnt[labels] > lo, c[:, b] - c[np.arange(n), labels], np.inf)
        i = int(d.argmin())
        cnt[labels[i]] -= 1
        labels[i] = b
        cnt[b] += 1
    return labels


def break_bound(c, labels, lo, hi, which):
    """The optimum with one point moved so that a count leaves [lo, hi] by one; None when no cluster sits on that bound
    (or k == 1)."""
    k = c.shape[1]
    cnt = np.bincount(labels, minlength=k)
    if k == 1:
        return None
    out = labels.copy()
    if which == "hi":
        full = np.flatnonzero(cnt == hi)
        if not len(full):
            return None
        b = int(full[0])
        out[np.flatnonzero(labels != b)[0]] = b
    else:
        low = np.flatnonzero(cnt == lo)
        if not len(low):
            return None
        a = int(low[0])
        out[np.flatnonzero(labels == a)[0]] = (a + 1) % k
    return out
