"""k-means++ seeding on the device (stdadk_kmeanspp_f64, contract in include/stdadk.h): the numpy float64 restatement of
that contract, the case tables and the comparator of tests/test_seed_cases_cpu.py and tests/test_gpu_knot_seeding.py.

The restatement follows sklearn's _kmeans_plusplus for unit weights with the random stream handed in: direct squared
distances, np.cumsum for the prefix sums, searchsorted(side='left') for the pick (clipped to n - 1), the first minimum
on ties.  Seeds are compared by COORDINATES, never by index: with duplicated sites another row of the same site is the
same seed, and only the seed rows' coordinates enter the fits.

Neither the library nor sklearn is imported here (make_seed_golden.py records sklearn's seeds into seed_*.npz).
"""
import functools
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_INIT = 3
RANDOM_STATE = 42

# the kernel's sizes (csrc/kmeanspp.hip): KPP_T threads, each owning 1, 2, 4, 7 or 10 rows in registers; beyond
# KPP_T * KPP_MAX_R rows the distances live in the workspace
KPP_T = 1024
KPP_ROWS = (1, 2, 4, 7, 10)
KPP_MAX_R = 10
KPP_MAX_L = 16
KPP_MAX_RUNS = 64
KPP_MAX_K = 65536


def trials(k):
    """sklearn's n_local_trials: 2 + floor(ln k) candidates per further centre."""
    return 2 + int(np.log(k))


def draw_stream(n, k, runs, seed=RANDOM_STATE, L=None):
    """(first (runs,) int32, u (runs, k - 1, L) float64) in the order sklearn's kmeans_plusplus draws from ONE
    RandomState(seed) over `runs` calls in sequence: the first row by choice(n, p = 1/n), then L uniforms per further
    centre."""
    rs = np.random.RandomState(seed)
    L = trials(k) if L is None else L
    p = np.ones(n, dtype=np.float64) / float(n)
    first, u = np.empty(runs, np.int32), np.empty((runs, k - 1, L), np.float64)
    for r in range(runs):
        first[r] = rs.choice(n, p=p)
        for c in range(k - 1):
            u[r, c] = rs.uniform(size=L)
    return first, u


def sqdist(X, c):
    """(x0 - c0)^2 + (x1 - c1)^2, every operation rounded once; c (2,) or (m, 2) -> (n,) or (m, n)."""
    c = np.asarray(c, np.float64)
    dx, dy = X[:, 0] - c[..., 0, None], X[:, 1] - c[..., 1, None]
    return dx * dx + dy * dy


def rows_per_thread(n):
    """Rows a thread of the kernel owns at n points."""
    per = -(-n // KPP_T)
    return next((r for r in KPP_ROWS if r >= per), per)


def kernel_order(v, rows):
    """The kernel's fixed summation order on v (..., n): (P (..., n) prefix sums, total (...)).  Chunks of `rows`
    consecutive terms added left to right from 0.0 (l), the 32 chunk sums of a group left to right (W exclusive), the
    32 group totals left to right (Gx exclusive): P = Gx + (W + l); the total is Gx + group total of the last group.
    np.cumsum adds left to right, one rounding per term."""
    v = np.asarray(v, np.float64)
    n, lead = v.shape[-1], v.shape[:-1]
    pad = np.zeros(lead + (KPP_T * rows,))
    pad[..., :n] = v
    l = np.cumsum(pad.reshape(lead + (32, 32, rows)), axis=-1)
    winc = np.cumsum(l[..., -1], axis=-1)                       # (..., 32, 32) inclusive over the chunks of a group
    W = np.concatenate([np.zeros(lead + (32, 1)), winc[..., :-1]], axis=-1)
    ginc = np.cumsum(winc[..., -1], axis=-1)                    # (..., 32) inclusive over the groups
    Gx = np.concatenate([np.zeros(lead + (1,)), ginc[..., :-1]], axis=-1)
    P = Gx[..., :, None, None] + (W[..., None] + l)
    return P.reshape(lead + (KPP_T * rows,))[..., :n], ginc[..., -1]


def restate(X, k, first, u, choose=None, rows=None):
    """One run of the contract: (rows (k,) int64, pot, picks (k,) the chosen candidate of every step, first_zero = the
    first step whose thresholds were formed on pot == 0, or k).  The sums are numpy's (np.cumsum for the prefix sums,
    np.sum for the potentials); with `rows` = rows_per_thread(n) they are formed in the kernel's own order instead
    (kernel_order), which the kernel must then match bit for bit -- the two differ only where a pick is decided by the
    rounding of a sum.  `choose(c, pots)` replaces the arg-min (the tests' deliberately wrong runs)."""
    X = np.asarray(X, np.float64)
    n = len(X)
    idx, picks, first_zero = np.empty(k, np.int64), np.zeros(k, np.int64), k
    idx[0] = first
    d = sqdist(X, X[first])
    P, pot = (np.cumsum(d), d.sum()) if rows is None else kernel_order(d, rows)
    pot = float(pot)
    for c in range(1, k):
        if pot == 0.0 and first_zero == k:
            first_zero = c
        r = u[c - 1] * pot
        cand = np.minimum(np.searchsorted(P, r, side="left"), n - 1)
        dc = np.minimum(d[None, :], sqdist(X, X[cand]))
        if rows is None:
            pots = dc.sum(axis=1)
        else:
            Pc, pots = kernel_order(dc, rows)
        j = int(np.argmin(pots)) if choose is None else int(choose(c, pots))
        idx[c], picks[c], d, pot = cand[j], j, dc[j], float(pots[j])
        P = np.cumsum(d) if rows is None else Pc[j]
    return idx, pot, picks, first_zero


def restate_runs(X, k, first, u, rows=None):
    """Every run of a call: (rows (runs, k), pots (runs,), first_zero (runs,))."""
    out = [restate(X, k, int(first[r]), u[r], rows=rows) for r in range(len(first))]
    return np.stack([o[0] for o in out]), np.asarray([o[1] for o in out]), np.asarray([o[3] for o in out])


def compare_seeds(X, got, want, what):
    """Seeds equal in coordinates, every run and every centre; returns how many indices differ (rows of one site)."""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.min() >= 0 and got.max() < len(X), (what, "seed row out of range", int(got.min()), int(got.max()))
    same = (X[got] == X[want]).all(axis=-1)
    if not same.all():
        where = np.argwhere(~same)[0]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} seeds differ in coordinates, the first at "
                             f"{tuple(int(w) for w in where)}: row {got[tuple(where)]} {X[got[tuple(where)]]} against "
                             f"row {want[tuple(where)]} {X[want[tuple(where)]]}")
    return int((got != want).sum())


def pot_bound(n, pot):
    """What two summation orders of n non-negative terms can differ by: n 2^-52 pot."""
    return n * 2.0 ** -52 * pot


# ------------------------------------------------------------------------------------------------ points
def points(family, n, seed, n_sites=500):
    """(n, 2) float64 in the unit square: 'uniform' (distinct rows); 'clustered' = five Gaussian blobs; 'sites' =
    n_sites sites x times (every row one of n_sites coordinates)."""
    rs = np.random.RandomState(seed)
    if family == "uniform":
        return rs.uniform(0.0, 1.0, (n, 2))
    if family == "sites":
        sites = rs.uniform(0.0, 1.0, (n_sites, 2))
        return sites[rs.randint(0, n_sites, n)]
    assert family == "clustered", family
    c = rs.uniform(0.15, 0.85, (5, 2))
    sig = rs.uniform(0.02, 0.08, 5)
    j = rs.randint(0, 5, n)
    return np.clip(c[j] + sig[j, None] * rs.standard_normal((n, 2)), 0.0, 1.0)


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------ kernel edge shapes
# (family, n, k, runs): n = 1, 2, 63, 64, 65, 1023, 1024, 1025, 10 000 and both sides of every change of the rows a thread
# owns (1 024 -> 2, 2 048 -> 4, 4 096 -> 7, 7 168 -> 10, 10 240 -> the workspace); k = 1, 2, a value at every change of
# L = trials(k) (3, 8, 21, 55, 149, 404, 1 097) and k = n on distinct points; runs = 1, 3 and 64.
_SHAPES = [
    ("uniform", 1, 1, 1), ("uniform", 2, 1, 3), ("uniform", 2, 2, 3), ("uniform", 63, 2, 1), ("uniform", 63, 8, 3),
    ("clustered", 64, 21, 3), ("uniform", 64, 64, 1), ("uniform", 65, 65, 3), ("clustered", 65, 55, 1),
    ("uniform", 1023, 149, 3), ("clustered", 1023, 3, 64), ("uniform", 1024, 404, 1), ("sites", 1024, 55, 3),
    ("uniform", 1025, 21, 64), ("clustered", 1025, 8, 3), ("uniform", 2048, 3, 1), ("clustered", 2049, 21, 3),
    ("uniform", 4096, 8, 3), ("sites", 4097, 55, 1), ("uniform", 7168, 21, 1), ("clustered", 7169, 8, 3),
    ("uniform", 2000, 1097, 1), ("uniform", 10000, 149, 3), ("clustered", 10000, 404, 1), ("sites", 10000, 55, 3),
    ("uniform", 10240, 8, 3), ("uniform", 10241, 8, 3), ("clustered", 20000, 21, 1), ("sites", 12000, 3, 64),
]
EDGE_CASES = [dict(name=f"{fam}_n{n}_k{k}_r{runs}", family=fam, n=n, k=k, runs=runs) for fam, n, k, runs in _SHAPES]
assert len({c["name"] for c in EDGE_CASES}) == len(EDGE_CASES)

# Cases whose data seed was replaced because a pick was decided by the rounding of a sum (profiles/knot_seeding.md).
# uniform_n2000_k1097_r1, first seed: at step 1087 the candidates rows 1593 and 534 are each other's only neighbours that
# the pick would move, so their potentials are equal in exact arithmetic; numpy's sums give ...1273 against ...1272 and
# the kernel's order gives both ...127 (restate(..., rows=2)): the tie falls to another candidate.
# seed_sites_n10000_k400, first seed: at step 85 of restart 0 the candidates rows 1478 and 3368 (two sites that are each
# other's nearest unchosen neighbour, with equally many rows) tie in the same way: numpy's sums give both ...732112,
# the kernel's order ...732116 against ...732112.
RESEEDED = {"uniform_n2000_k1097_r1": 1, "seed_sites_n10000_k400": 1}

# duplicated sites with k above the number of distinct points: (n, sites, k, runs)
DEGENERATE_CASES = [dict(name=f"degenerate_n{n}_s{s}_k{k}_r{runs}", n=n, sites=s, k=k, runs=runs)
                    for n, s, k, runs in ((300, 20, 40, 3), (1500, 7, 21, 1), (5, 1, 5, 3))]


@functools.lru_cache(maxsize=None)
def edge_inputs(name):
    """dict(X, first, u, L) of an edge case; the stream is drawn as sklearn would, from a seed of the case's own."""
    case = next(c for c in EDGE_CASES if c["name"] == name)
    seeded = name + (f"/{RESEEDED[name]}" if name in RESEEDED else "")
    X = points(case["family"], case["n"], _seed(seeded), n_sites=max(case["k"] + 5, case["n"] // 20))
    first, u = draw_stream(case["n"], case["k"], case["runs"], seed=_seed(seeded + "/stream"))
    return dict(X=X, first=first, u=u, L=u.shape[2])


@functools.lru_cache(maxsize=None)
def degenerate_inputs(name):
    case = next(c for c in DEGENERATE_CASES if c["name"] == name)
    X = points("sites", case["n"], _seed(name), n_sites=case["sites"])
    first, u = draw_stream(case["n"], case["k"], case["runs"], seed=_seed(name + "/stream"))
    return dict(X=X, first=first, u=u, L=u.shape[2], distinct=len(np.unique(X, axis=0)))


@functools.lru_cache(maxsize=None)
def edge_expected(name, kernel_sums=False):
    """The restatement on an edge or degenerate case, computed once: (rows (runs, k), pots (runs,), first_zero (runs,));
    kernel_sums: the sums in the kernel's order."""
    inp = degenerate_inputs(name) if name.startswith("degenerate") else edge_inputs(name)
    return restate_runs(inp["X"], inp["u"].shape[1] + 1, inp["first"], inp["u"],
                        rows=rows_per_thread(len(inp["X"])) if kernel_sums else None)


# ------------------------------------------------------------------------------------------------ sklearn's seeds
# recorded by make_seed_golden.py with the installed sklearn: (family, n, k, sites)
NEW_SKLEARN_CASES = [dict(name=f"seed_{fam}_n{n}_k{k}", family=fam, n=n, k=k, sites=s)
                     for fam, n, k, s in (("uniform", 10000, 121, 0), ("clustered", 10000, 121, 0),
                                          ("sites", 10000, 400, 500), ("clustered", 10000, 1024, 0))]
# the fits' fixtures already hold X and sklearn's three seed sets of one RandomState(42)
OLD_SKLEARN_FILES = [f"gmm_fit_{fam}_k{k}" for fam in ("clustered", "sites", "uniform") for k in (25, 81)] + \
                    [f"kmeans_fit_{fam}_k{k}" for fam in ("clustered", "sites", "uniform") for k in (9, 25)]
SKLEARN_CASES = [c["name"] for c in NEW_SKLEARN_CASES] + OLD_SKLEARN_FILES


def new_case_points(case):
    name = case["name"]
    return points(case["family"], case["n"], _seed(name + (f"/{RESEEDED[name]}" if name in RESEEDED else "")),
                  n_sites=case["sites"] or 500)


@functools.lru_cache(maxsize=None)
def sklearn_case(name):
    """dict(X, seeds (3, k) sklearn's rows, first, u) of a recorded case; for the older fixtures the stream is drawn here."""
    fx = np.load(os.path.join(HERE, name + ".npz"))
    X, seeds = fx["X"], fx["seeds"].astype(np.int64)
    if "u" in fx.files:
        first, u = fx["first"], fx["u"]
    else:
        first, u = draw_stream(len(X), seeds.shape[1], len(seeds))
    return dict(X=X, seeds=seeds, first=first, u=u)
