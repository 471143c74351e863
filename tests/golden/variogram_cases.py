"""Empirical space-time variograms (stdadk_variogram_f32, Predictor.variogram_grid, stnf.utils.variogram, grid_scores'
`variogram` entry): the tests' own restatements of the contract in include/stdadk.h, the bound, the comparator, the
case generator and the end-to-end model.  Shared by tests/test_variogram_cases_cpu.py (runs anywhere) and
tests/test_gpu_variogram.py.  Not imported by the product.

CONTRACT, restated.  An entry (t, s) is counted when z[t][s] is finite and its code is 0..3.  For lag u and
t = 0 .. nT-1-u a pair is a = (t, i), b = (t + u, j): i < j at u = 0, every ordered (i, j) at u > 0.  It counts in split
c when both entries are counted with code c, in bin b when edges2[b] <= d2 < edges2[b+1], d2 = dx dx + dy dy in
float64 from the float32 coordinates, every operation rounded once.  acc[c][u][b] = (N, SZ, SP, SR): the count and the
sums of (z_a - z_b)^2, (p_a - p_b)^2, ((z_a - p_a) - (z_b - p_b))^2, each formed in double.  Without a prediction SP
and SR are 0.

THREE RESTATEMENTS.
  restate_brute   plain Python loops over (u, t, i, j); every term collected and added with math.fsum: exact.  `hook`
                  lets a test miscount on purpose (the comparator's teeth).
  restate_exact   the same terms formed by numpy float64 elementwise (the same IEEE operations, hence the same bits),
                  grouped by (split, bin) and added with math.fsum: exact, and fast enough for the kernel's shapes.
  restate_numpy   vectorised, sums by numpy (bincount): not exact; for the mid-size case.

BOUND.  A slot's sum is of N non-negative doubles.  Adding them in ANY order, with or without the square fused into the
sum, every partial sum carries a relative error of at most 2^-53 and there are at most N roundings on the way of any
term, so |dev - exact| <= N 2^-52 exact (first order with a factor 2 to spare).  Against restate_numpy, whose own sum
is off by as much, the bound is twice that.  N is EXACT always.
"""
import math

import numpy as np

N_, SZ, SP, SR = 0, 1, 2, 3
MAX_BINS, MAX_LAGS = 64, 16
TILE = 16                                       # VG_E of csrc/variogram.hip (pinned by the CPU test against the source)

SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
SLICES = [1, 2, 7]
LAGS = [1, 2, 7, 9]
BINS = [1, 5, 64]


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _codes(z, split):
    """Per entry the split code 0..3 of a counted entry, -1 otherwise."""
    z = np.asarray(z, dtype=np.float32)
    code = np.zeros(z.shape, dtype=np.int64) if split is None else np.asarray(split).astype(np.int64)
    return np.where(np.isfinite(z) & (code >= 0) & (code <= 3), code, -1)


def sq_dist(coords):
    """d2 (S, S) float64: two differences, two products, one sum, each rounded once."""
    x = _f64(coords)
    dx, dy = x[:, None, 0] - x[None, :, 0], x[:, None, 1] - x[None, :, 1]
    return dx * dx + dy * dy


def bin_of(d2, edges2):
    """The bin of d2 under the half-open rule, -1 for none; scalar, by the definition itself."""
    for b in range(len(edges2) - 1):
        if edges2[b] <= d2 < edges2[b + 1]:
            return b
    return -1


# ------------------------------------------------------------------------------------------------ restatements
def restate_brute(pred, z, split, coords, edges2, n_lags, hook=None):
    """acc (4, L, B, 4) by plain loops and math.fsum.  pred (T, S) or None.  `hook(u, t, i, j, b)` returns the bins the
    pair is counted in (default [b]): the way a test builds a WRONG answer."""
    z32 = np.asarray(z, dtype=np.float32)
    T, S = z32.shape
    B, L = len(edges2) - 1, int(n_lags)
    code = _codes(z32, split).tolist()
    zz = z32.astype(np.float64).tolist()
    pp = None if pred is None else _f64(pred).tolist()
    xy = _f64(coords).tolist()
    terms = {}
    for i in range(S):
        for j in range(S):
            dx, dy = xy[i][0] - xy[j][0], xy[i][1] - xy[j][1]
            b = bin_of(dx * dx + dy * dy, edges2)
            if b < 0:
                continue
            for u in range(L):
                if u == 0 and not i < j:
                    continue
                for t in range(T - u):
                    c = code[t][i]
                    if c < 0 or c != code[t + u][j]:
                        continue
                    dz = zz[t][i] - zz[t + u][j]
                    tp = tr = 0.0
                    if pp is not None:
                        dp = pp[t][i] - pp[t + u][j]
                        dr = (zz[t][i] - pp[t][i]) - (zz[t + u][j] - pp[t + u][j])
                        tp, tr = dp * dp, dr * dr
                    for bb in ([b] if hook is None else hook(u, t, i, j, b)):
                        terms.setdefault((c, u, bb), []).append((dz * dz, tp, tr))
    acc = np.zeros((4, L, B, 4))
    for (c, u, b), rows in terms.items():
        acc[c, u, b] = [len(rows)] + [math.fsum(r[k] for r in rows) for k in range(3)]
    return acc


def _pair_slices(pred, z, split, coords, edges2, n_lags):
    """Yields (u, key (n,), tz (n,), tp (n,), tr (n,)) per (u, t): key = split * B + bin of the counting pairs, the
    terms formed elementwise in float64."""
    z32 = np.asarray(z, dtype=np.float32)
    T, S = z32.shape
    e2 = np.asarray(edges2, dtype=np.float64)
    B = len(e2) - 1
    code = _codes(z32, split)
    zd = np.where(code >= 0, z32, 0).astype(np.float64)
    pd = None if pred is None else _f64(pred)
    d2 = sq_dist(coords)
    pair_bin = np.full((S, S), -1, dtype=np.int64)
    for b in range(B):                                            # the rule itself, bin by bin
        pair_bin[(e2[b] <= d2) & (d2 < e2[b + 1])] = b
    upper = np.arange(S)[:, None] < np.arange(S)[None, :]
    for u in range(min(int(n_lags), T)):
        pb = np.where(upper, pair_bin, -1) if u == 0 else pair_bin
        for t in range(T - u):
            ca, cb = code[t][:, None], code[t + u][None, :]
            m = (ca == cb) & (ca >= 0) & (pb >= 0)
            ii, jj = np.nonzero(m)
            key = code[t][ii] * B + pb[ii, jj]
            dz = zd[t][ii] - zd[t + u][jj]
            if pd is None:
                tp = tr = np.zeros(len(ii))
            else:
                dp = pd[t][ii] - pd[t + u][jj]
                dr = (zd[t][ii] - pd[t][ii]) - (zd[t + u][jj] - pd[t + u][jj])
                tp, tr = dp * dp, dr * dr
            yield u, key, dz * dz, tp, tr


def restate_exact(pred, z, split, coords, edges2, n_lags):
    """acc (4, L, B, 4): numpy forms the terms, math.fsum adds each (split, lag, bin) group."""
    B, L = len(edges2) - 1, int(n_lags)
    per_lag = [[] for _ in range(L)]
    for u, key, tz, tp, tr in _pair_slices(pred, z, split, coords, edges2, L):
        per_lag[u].append((key, tz, tp, tr))
    acc = np.zeros((4, L, B, 4))
    for u, parts in enumerate(per_lag):
        if not parts:
            continue
        key = np.concatenate([p[0] for p in parts])
        order = np.argsort(key, kind="stable")
        key = key[order]
        cuts = np.nonzero(np.diff(key))[0] + 1
        starts = np.concatenate([[0], cuts]) if len(key) else []
        ends = np.concatenate([cuts, [len(key)]]) if len(key) else []
        cols = [np.concatenate([p[k] for p in parts])[order] for k in (1, 2, 3)]
        for s, e in zip(starts, ends):
            c, b = divmod(int(key[s]), B)
            acc[c, u, b] = [e - s] + [math.fsum(col[s:e].tolist()) for col in cols]
    return acc


def restate_numpy(pred, z, split, coords, edges2, n_lags):
    """acc (4, L, B, 4) with numpy's own sums (bincount)."""
    B, L = len(edges2) - 1, int(n_lags)
    acc = np.zeros((4, L, B, 4))
    for u, key, tz, tp, tr in _pair_slices(pred, z, split, coords, edges2, L):
        acc[:, u, :, N_] += np.bincount(key, minlength=4 * B).reshape(4, B)
        for k, w in ((SZ, tz), (SP, tp), (SR, tr)):
            acc[:, u, :, k] += np.bincount(key, weights=w, minlength=4 * B).reshape(4, B)
    return acc


# ------------------------------------------------------------------------------------------------ the comparator
def compare(got, ref, factor=1.0):
    """`got` against `ref` (4, L, B, 4): every N EXACT, every sum within factor x N 2^-52 ref (factor 2 when ref is
    itself a numpy sum).  Returns the list of failures, empty when the two agree."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return [f"shape {got.shape} vs {ref.shape}"]
    bad = []
    n = ref[..., N_]
    tol = np.zeros(ref.shape)
    tol[..., 1:] = (factor * n * 2.0 ** -52)[..., None] * np.abs(ref[..., 1:])
    for c, u, b, k in zip(*np.nonzero(~(np.abs(got - ref) <= tol))):
        bad.append(f"split {c} lag {u} bin {b} slot {k}: {got[c, u, b, k]!r} vs {ref[c, u, b, k]!r} "
                   f"(bound {tol[c, u, b, k]:.3e})")
    return bad


# ------------------------------------------------------------------------------------------------ the case generator
def make_case(S, nT, seed=0, ldy=1, spread=32):
    """(y_pred (nT*S, ldy) float32, z (nT, S) float32, split (nT, S) uint8, coords (S, 2) float32).  Coordinates on a
    lattice of eighths in [0, spread / 8) (d2 is exact; duplicated sites occur, and the first two sites ARE duplicates
    when S >= 2); z multiples of 1/16 with about a tenth NaN / +inf / -inf; predictions multiples of 1/8; codes 0..3
    with an invalid 7 now and then."""
    rs = np.random.RandomState(7919 * seed + 101 * S + nT)
    coords = rs.randint(0, spread, size=(S, 2)) / 8.0
    if S >= 2:
        coords[1] = coords[0]
    z = rs.randint(-80, 81, size=(nT, S)) / 16.0
    w = rs.uniform(size=(nT, S))
    z = np.select([w < 0.04, w < 0.07, w < 0.1], [np.nan, np.inf, -np.inf], z)
    y = rs.randint(-64, 65, size=(nT * S, ldy)) / 8.0
    code = np.where(rs.uniform(size=(nT, S)) < 0.06, 7, rs.randint(0, 4, size=(nT, S)))
    return y.astype(np.float32), z.astype(np.float32), code.astype(np.uint8), coords.astype(np.float32)


def edges_on_attained(coords, n_bins, first_zero=True):
    """n_bins + 1 squared edges placed ON attained values of d2 wherever the case has enough of them (the half-open
    rule then decides pairs on both sides of every edge), the last edge below the largest attained value when it can
    be (pairs at or beyond it count nowhere).  first_zero=False: edges2[0] is the smallest POSITIVE attained value, so
    that i = j and duplicated sites count nowhere."""
    vals = np.unique(sq_dist(coords))
    vals = vals[np.isfinite(vals)]
    if not first_zero:
        vals = vals[vals > 0]
    pool = vals[:-1] if len(vals) > n_bins + 1 else vals
    pick = np.unique(np.round(np.linspace(0, len(pool) - 1, n_bins + 1)).astype(int)) if len(pool) else []
    e = [float(pool[k]) for k in pick]
    if not e:
        e = [0.0 if first_zero else 0.015625]
    while len(e) < n_bins + 1:                                     # too few attained values: go on past them
        e.append(e[-1] + 0.015625 * (1 + len(e) % 3))
    e = np.asarray(e[:n_bins + 1], dtype=np.float64)
    assert (np.diff(e) > 0).all() and e[0] >= 0
    return e


def toggles(k):
    """(split given, prediction: None / (ldy, col), edges2[0] == 0) of the k-th kernel run: cycles through all."""
    pred = [None, (5, 4), (5, 0), (1, 0)][k % 4]
    return bool((k // 4) % 2 == 0), pred, bool((k // 8) % 3 != 0)


# ------------------------------------------------------------------------------------------------ end to end
E2E_S, E2E_T, E2E_SEED = 70, 9, 5


def e2e_model(hidden=(32, 16), output_dim=3, seed=E2E_SEED):
    """A freshly initialised model (torch.manual_seed(seed)): [25] spatial knots, [10] temporal, hidden [32, 16]."""
    import torch
    from stnf.models import STInterpMLP
    torch.manual_seed(seed)
    return STInterpMLP(p=0, k_spatial_centers=[25], k_temporal_centers=[10], hidden_dims=list(hidden), dropout=0.0,
                       layernorm=True, output_dim=output_dim).eval()


def e2e_field(seed=78, S=E2E_S, T=E2E_T):
    """coords (S, 2) in the unit square, z (T, S) float32 with about 15 % NaN, a +inf and a -inf, codes 0..3."""
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = (0.3 * rs.standard_normal((T, S))).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.15] = np.nan
    z[0, 0], z[T - 1, S - 1] = np.inf, -np.inf
    code = rs.randint(0, 4, size=(T, S)).astype(np.uint8)
    return coords, z, code


def grid_times(T):
    """grid_scores' times as float32: t_idx / (T - 1)."""
    return (np.arange(T, dtype=np.float32) / np.float32(T - 1)) if T > 1 else np.zeros(1, dtype=np.float32)
