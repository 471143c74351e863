"""Local ordinary kriging (stdadk_krige_weights_f64, stdadk_krige_apply_f32, stnf.utils.kriging): the case generator, the
tests' own long-double restatement and the comparators.  Shared by tests/test_kriging_cases_cpu.py (runs anywhere),
tests/test_gpu_kriging.py and tests/golden/make_kriging_achieved.py.  Not imported by the product; no stored arrays.

CONTRACT (include/stdadk.h), restated.  Of a table row the entries that count (0 <= idx < S) are taken in row order;
entries whose sources are at squared distance exactly 0 form a group, one unknown, represented by its first member.
K_ab = psill rho(d_ab) + [a == b] nugget / members_a, k_a = psill rho(d_a0); mu = (sum K^-1 k - 1) / sum K^-1 1,
w = K^-1 k - mu K^-1 1, var = nugget + psill - w.k - mu; a group's weight goes to every member as w / members.

COMPARISON.  `reference` solves, per row and in np.longdouble, the full BORDERED system [[K, 1], [1^T, 0]] [w; mu] =
[k; 1] by Gaussian elimination with partial pivoting, rho evaluated in long double from the table's d2 and from
pairwise d2 formed in long double (differences of float32 coordinates, exact there).  It shares no line with the
product.  The product's float64 Cholesky is held to

    |w - w_ref| <= c(n) kappa 2^-52 max(1, max|w_ref|)   per row,   c(n) = 4 n (3 n + 1) + 8 n,

with n unknowns and kappa = |K|_inf |K^-1|_inf in long double.  Reasoning: a Cholesky solve is backward stable with
|dK|_2 <= 4 n (3 n + 1) u |K|_2 (Higham, Accuracy and Stability, thm 10.4 with 10.5's norm bound), which moves the
solution by that times kappa, relatively; every entry of K and k carries at most 4 roundings of its own (the square
root, the division by the range, exp or the polynomial's last operation, the product with psill) and the diagonal two,
at most 8 n u |K| in the infinity norm.  w is a difference of two such solutions, of size comparable to the largest
weight or to 1 (the weights sum to 1).  var = C00 - sum w_a k_a - mu with |k_a| <= psill, and mu the bordered unknown in
units of covariance: (n + 1) (nugget + psill) times the weights' bound.
On the device the spherical model repeats the host's bits; exp differs in its last bits between the libraries, so the
exponential and gaussian models are held to K_exp kappa 2^-52 max|w| per row with K_exp MEASURED on the host
(make_kriging_achieved.py -> kriging_achieved.json) on the cases with kappa <= KAPPA_MAX, a condition of the generator.
"""
import numpy as np

L = np.longdouble
MAX_K = 16
KAPPA_MAX = 1e9                                  # the bounded (exponential / gaussian) cases stay below this
MODELS = ("exponential", "spherical", "gaussian")
SIZES_M = [1, 3, 4, 5, 63, 64, 65, 257]          # the rows-per-wave (4 at 16 lanes) and workgroup (16, 32, 64 rows) seams
SIZES_K = [1, 2, 8, 15, 16]
KINDS = ("uniform", "lattice")


def points(rs, n, kind):
    """n float32 points: uniform in the unit square, or a LATTICE of spacing 1/4 with repeated points (coincident
    sources and equal distances are the rule there)."""
    if kind == "uniform":
        return rs.uniform(0, 1, (n, 2)).astype(np.float32)
    return (rs.randint(0, 5, (n, 2)) / 4.0).astype(np.float32)


def make_case(M, S, k, nM=1, kind="uniform", model="spherical", nugget=0.1, psill=1.0, range_=0.5, counts=None, seed=0,
              k_tab=None):
    """One case as a dict: q (M, 2), coords (S, 2) float32, src (nM, S) uint8 or None (every site), k_tab, k, the model
    and its parameters, z (nT, S) float32 with nT = nM, or 3 for one slice.  `counts`: sources per slice (the rest of
    the row is the search's -1 tail).  Every fifth target lies ON a source."""
    rs = np.random.RandomState(104729 * seed + 131 * M + 17 * S + 3 * k + nM)
    coords = points(rs, S, kind)
    q = points(rs, M, kind)
    q[::5] = coords[rs.randint(S, size=len(q[::5]))]
    src = None
    if counts is not None or nM > 1:
        counts = [S] * nM if counts is None else counts
        src = np.zeros((nM, S), dtype=np.uint8)
        for m, n in enumerate(counts):
            src[m, rs.permutation(S)[:n]] = 1
    nT = nM if nM > 1 else 3
    z = rs.standard_normal((nT, S)).astype(np.float32)
    return dict(q=q, coords=coords, src=src, k=k, k_tab=min(MAX_K, k + 1) if k_tab is None else k_tab, model=model,
                nugget=float(nugget), psill=float(psill), range=float(range_), z=z)


def group_case():
    """Coincident groups of 2 and 3 that are NOT adjacent in their row: the target at the origin, sources 0, 2, 4 at
    (1/2, 0) and 1, 3 at (0, 1/2) -- all at the same distance, so the row is in index order 0 1 2 3 4 -- then two more."""
    coords = np.asarray([[.5, 0], [0, .5], [.5, 0], [0, .5], [.5, 0], [.75, .25], [.25, 1.0]], dtype=np.float32)
    q = np.asarray([[0, 0], [.5, 0], [.25, .25]], dtype=np.float32)
    z = np.random.RandomState(3).standard_normal((3, 7)).astype(np.float32)
    return dict(q=q, coords=coords, src=None, k=7, k_tab=8, model="spherical", nugget=0.25, psill=1.0, range=2.0, z=z)


def singular_case():
    """Gaussian, nugget 0, a range so far above the neighbourhood that every rho rounds to exactly 1 (r^2 <= 1e-24, in
    float64 and in long double alike): K is psill times the all-ones matrix and the second pivot is 1 - 1 * 1 = 0.
    k = 1 rows would be regular; k = 8 makes every row singular."""
    return make_case(65, 40, 8, model="gaussian", nugget=0.0, range_=1e13, seed=77)


def bitwise_cases():
    """The cases whose device output repeats the host's bits: the spherical model on every M and k, both kinds of
    coordinates, nugget 0 and > 0, shared and per-slice tables, short rows (0, 1, 2 and k - 1 sources), a range below
    the nearest distance (K = diagonal), a range far above the neighbourhood (ill-conditioned); the crafted groups; the
    singular case."""
    out = []
    for n, M in enumerate(SIZES_M):
        k = SIZES_K[n % 5]
        out.append(make_case(M, 40, k, kind=KINDS[n % 2], nugget=(0.0, 0.1)[n % 2], seed=n))
    for n, k in enumerate(SIZES_K):
        out.append(make_case(65, 60, k, kind=KINDS[(n + 1) % 2], nugget=(0.2, 0.0)[n % 2], range_=0.8, seed=20 + n))
    out.append(make_case(5, 40, 8, nM=3, counts=[7, 2, 0], seed=30))
    out.append(make_case(65, 40, 15, nM=3, counts=[14, 1, 40], kind="lattice", seed=31))
    out.append(make_case(64, 50, 8, range_=1e-4, seed=32))                 # below the nearest distance: rho = 0
    out.append(make_case(64, 50, 8, range_=1e-4, nugget=0.0, seed=33))
    out.append(make_case(63, 50, 16, range_=300.0, seed=34))               # far above the neighbourhood
    out.append(make_case(63, 50, 16, range_=300.0, nugget=0.0, seed=35))
    out.append(group_case())
    out.append(singular_case())
    return out


def bounded_cases():
    """The exponential and gaussian cases of the device comparison, kappa <= KAPPA_MAX in every row (asserted by the CPU
    test): every k, both kinds, nugget 0 and > 0, shared and per-slice tables with short rows, small and large ranges."""
    out = []
    for n, k in enumerate(SIZES_K):
        out.append(make_case(SIZES_M[n + 3], 40, k, kind=KINDS[n % 2], model="exponential", nugget=(0.0, 0.1)[n % 2],
                             range_=0.4, seed=40 + n))
        out.append(make_case(65, 40, k, kind=KINDS[(n + 1) % 2], model="gaussian", nugget=0.05, range_=0.15, seed=50 + n))
    out.append(make_case(65, 40, 8, nM=3, counts=[7, 2, 0], model="exponential", seed=60))
    out.append(make_case(64, 50, 16, model="exponential", range_=1e-4, seed=61))
    out.append(make_case(64, 50, 16, model="exponential", nugget=0.0, range_=50.0, seed=62))      # ill-conditioned
    out.append(make_case(64, 50, 8, model="gaussian", nugget=0.0, range_=0.05, seed=63))
    return out


def all_cases():
    return bitwise_cases() + bounded_cases()


def table(case):
    """The case's neighbour table from knn_host: (nbr_idx, nbr_d2), (nM, M, k_tab)."""
    from stnf.utils import baselines as BL
    return BL.knn_host(case["q"], case["coords"], case["src"], case["k_tab"], False)


# ---- the independent restatement ---------------------------------------------------------------

def rho_ld(model, d, range_):
    r = d / L(range_)
    if model == "exponential":
        return np.exp(-r)
    if model == "gaussian":
        return np.exp(-(r * r))
    return L(1) - r * (L(1.5) - L(0.5) * r * r) if d < L(range_) else L(0)


def solve_ld(A, B):
    """A^-1 B in long double by Gaussian elimination with partial pivoting; None when a pivot is exactly 0."""
    A, B = np.array(A, dtype=L), np.array(B, dtype=L)
    n = len(A)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if A[p, c] == 0:
            return None
        A[[c, p]], B[[c, p]] = A[[p, c]], B[[p, c]]
        for r in range(c + 1, n):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            B[r] -= f * B[c]
    X = np.zeros_like(B)
    for r in range(n - 1, -1, -1):
        X[r] = (B[r] - A[r, r + 1:] @ X[r + 1:]) / A[r, r]
    return X


def row_system(case, idx_row, d2_row, collapse=True):
    """Of one table row: (entries, groups, K, kvec) in long double.  entries: positions that count; groups: per unknown
    the list of positions (every position its own group when not collapsed); K without any border."""
    S, c = len(case["coords"]), case["coords"].astype(L)
    ent = [e for e in range(case["k"]) if 0 <= idx_row[e] < S]
    groups = []
    for e in ent:
        home = None
        if collapse:
            for g in groups:
                if (c[idx_row[g[0]]] == c[idx_row[e]]).all():
                    home = g
                    break
        if home is None:
            groups.append([e])
        else:
            home.append(e)
    n = len(groups)
    K, kv = np.zeros((n, n), dtype=L), np.zeros(n, dtype=L)
    for a, ga in enumerate(groups):
        pa = c[idx_row[ga[0]]]
        kv[a] = L(case["psill"]) * rho_ld(case["model"], np.sqrt(L(d2_row[ga[0]])), case["range"])
        for b, gb in enumerate(groups):
            pb = c[idx_row[gb[0]]]
            d = np.sqrt((pa[0] - pb[0]) ** 2 + (pa[1] - pb[1]) ** 2)
            K[a, b] = L(case["psill"]) * rho_ld(case["model"], d, case["range"])
        K[a, a] = L(case["psill"]) + L(case["nugget"]) / L(len(ga))
    return ent, groups, K, kv


def reference(case, tab=None, collapse=True):
    """The long-double answer of every row: w (nM, M, k) and var (nM, M) as longdouble, kappa (nM, M) and n (nM, M) the
    unknowns.  A row with no entry: w = 0, var = NaN, kappa = 0.  A row whose elimination meets a pivot of exactly 0:
    all NaN, kappa = inf."""
    idx, d2 = table(case) if tab is None else tab
    nM, M, _ = idx.shape
    k = case["k"]
    w, var = np.zeros((nM, M, k), dtype=L), np.full((nM, M), np.nan, dtype=L)
    kappa, unknowns = np.zeros((nM, M)), np.zeros((nM, M), dtype=np.int64)
    for m in range(nM):
        for j in range(M):
            ent, groups, K, kv = row_system(case, idx[m, j], d2[m, j], collapse)
            n = len(groups)
            unknowns[m, j] = n
            if n == 0:
                continue
            inv = solve_ld(K, np.eye(n, dtype=L))
            A = np.zeros((n + 1, n + 1), dtype=L)
            A[:n, :n], A[:n, n], A[n, :n] = K, 1, 1
            sol = None if inv is None else solve_ld(A, np.concatenate([kv, [L(1)]])[:, None])
            if sol is None:
                w[m, j], kappa[m, j] = np.nan, np.inf
                continue
            kappa[m, j] = float(np.abs(K).sum(axis=1).max() * np.abs(inv).sum(axis=1).max())
            wg, mu = sol[:n, 0], sol[n, 0]
            var[m, j] = L(case["nugget"]) + L(case["psill"]) - wg @ kv - mu
            for g, members in enumerate(groups):
                for e in members:
                    w[m, j, e] = wg[g] / L(len(members))
    return w, var, kappa, unknowns


def c_of(n):
    return 4.0 * n * (3.0 * n + 1.0) + 8.0 * n


def weight_bounds(case, ref):
    """Per row the bound on |w - w_ref| and on |var - var_ref| of the head comment, float64 (inf where kappa is)."""
    w, _, kappa, n = ref
    with np.errstate(invalid="ignore"):
        wmax = np.maximum(1.0, np.nan_to_num(np.abs(w).max(axis=2).astype(np.float64), nan=1.0))
    bw = c_of(n) * kappa * 2.0 ** -52 * wmax
    return bw, bw * (n + 1) * (case["nugget"] + case["psill"])


def close_to_reference(case, w, var, ref):
    """Whether the float64 answer (w, var) is within the bounds of the reference, NaN patterns apart: a reference row of
    NaN (exactly singular) must be NaN; a product row of NaN is accepted only where the bound exceeds 1 (the row is
    numerically singular).  Returns (ok, worst ratio of an error to its bound)."""
    rw, rv, kappa, n = ref
    bw, bv = weight_bounds(case, ref)
    ok, worst = True, 0.0
    for m, j in np.ndindex(*kappa.shape):
        if n[m, j] == 0:
            ok &= bool((w[m, j] == 0).all() and np.isnan(var[m, j]))
        elif not np.isfinite(kappa[m, j]):
            ok &= bool(np.isnan(w[m, j]).all() and np.isnan(var[m, j]))
        elif np.isnan(var[m, j]) or np.isnan(w[m, j]).any():
            ok &= bool(bw[m, j] > 1.0 and np.isnan(w[m, j]).all() and np.isnan(var[m, j]))
        else:
            ew = float(np.abs(w[m, j].astype(L) - rw[m, j]).max())
            ev = float(abs(L(var[m, j]) - rv[m, j]))
            ok &= ew <= bw[m, j] and ev <= bv[m, j]
            worst = max(worst, ew / bw[m, j], ev / bv[m, j])
    return ok, worst


def apply_reference(case, tab_idx, w, var, zq):
    """stdadk_krige_apply_f32 in long double from float64 w and var: (out (nT, M, Q) longdouble, scale (nT, M) =
    sum |w z| + max|zq| sd, the magnitude the rounding errors are relative to)."""
    z = case["z"]
    nT, S = z.shape
    nM, M, _ = tab_idx.shape
    out, scale = np.full((nT, M, len(zq)), np.nan, dtype=L), np.zeros((nT, M), dtype=L)
    for ti in range(nT):
        m = 0 if nM == 1 else ti
        for j in range(M):
            if np.isnan(var[m, j]):
                continue
            ent = [e for e in range(case["k"]) if 0 <= tab_idx[m, j, e] < S]
            p = sum((L(w[m, j, e]) * L(z[ti, tab_idx[m, j, e]]) for e in ent), L(0))
            sd = np.sqrt(L(max(var[m, j], 0.0)))
            out[ti, j] = p + np.asarray(zq, dtype=L) * sd
            scale[ti, j] = sum((abs(L(w[m, j, e]) * L(z[ti, tab_idx[m, j, e]])) for e in ent), L(0)) + \
                L(np.abs(zq).max()) * sd
    return out, scale


def same_bits(a, b):
    """Equal shapes, dtypes and bits, every NaN matching a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.array_equal(np.isnan(a), np.isnan(b))) and \
        bool(np.array_equal(np.where(np.isnan(a), 0, a).view(f"u{a.itemsize}"), np.where(np.isnan(b), 0, b).view(f"u{b.itemsize}")))


def within_exp_bound(w, var, host_w, host_var, kappa, k_exp, c00):
    """The device's (w, var) against the host's for the models that go through exp: the same NaN positions, and per
    row |w - w_host| <= K_exp kappa 2^-52 max|w_host|, the variance within that times (k + 1) C00.  Returns (ok, worst
    ratio)."""
    if not (np.array_equal(np.isnan(w), np.isnan(host_w)) and np.array_equal(np.isnan(var), np.isnan(host_var))):
        return False, np.inf
    k = w.shape[2]
    with np.errstate(invalid="ignore"):
        bound = k_exp * kappa * 2.0 ** -52 * np.nan_to_num(np.abs(host_w).max(axis=2), nan=0.0)
        ew = np.nan_to_num(np.abs(w - host_w).max(axis=2), nan=0.0)
        ev = np.nan_to_num(np.abs(var - host_var), nan=0.0)
    ok = bool((ew <= bound).all() and (ev <= bound * (k + 1) * c00).all())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, ew / np.where(bound > 0, bound, 1.0), np.where(ew > 0, np.inf, 0.0))
    return ok, float(ratio.max()) if ratio.size else 0.0
