"""Quantile diagnostics (stdadk_quantile_diag_f32, Predictor.quantile_grid, grid_scores' `quantile` entry, Evaluator's
`diagnostics`): the tests' own numpy float64 restatement of the contract in include/stdadk.h, the derived bound of the
float sums, the comparator, the case generator and the end-to-end model.  Shared by tests/test_quantile_diag_cases_cpu.py
(runs anywhere) and tests/test_gpu_quantile_diag.py.  Not imported by the product.

RESTATEMENT.  `restate(y_pred, z, split, ...)` returns (split_acc (4, SLOTS), site_acc (4, S, 4), time_acc (4, T, 4)).
Every count is an integer.  Every float sum is the EXACT sum (math.fsum) of terms formed as the contract forms them, in
double from operands converted to double, every operation rounded once:
    crps term of an entry    (2 / Q) * (((rho_0 + rho_1) + ...) + rho_Q-1),  rho_q = max((tau_q - 1) e, tau_q e), e = z - p_q
    depth terms of an entry  max(0, p_q - p_q+1) and its square, one of each per adjacent pair
so the restatement itself adds no summation error, and the whole distance to the device is the device's.

BOUND.  The device adds n such terms in an order of its own (lanes, waves, workgroups, slices).  Any order of adding n
numbers in double is off the exact sum by at most (n - 1) u sum|term| to first order, u = 2^-53; the contract's bound
is |delta| <= (n + 3) 2^-53 sum|term|, with n the number of terms of the group (entries for CRPS, entries x pairs for
the depths; terms that are exactly 0 -- masked lanes -- add nothing).  `bounds(...)` computes it from the case's own
terms, per slot, per site and per time, the way eval_cases derives its reduction bound.

CASES.  `make_case(S, nT, Q, seed)` writes the prediction rows directly (multiples of 1/8; z multiples of 1/16), so
every predicate is decided on exactly representable float32 values.  A case with at least 64 entries contains, in every
split code 0..3: strictly sorted rows, rows with exactly one crossing at each adjacent pair, fully reversed rows, rows
with equal neighbours, entries with z exactly equal to some p_q, NaN, +inf and -inf values of z; and entries with
split code 7.  `conditions(...)` reads them back from the arrays (not from the generator's bookkeeping).
"""
import math

import numpy as np

# the STDADK_QD_* slots of include/stdadk.h, restated
MAX_Q = 8
N_, BELOW, PIT, CROSS_ROWS, PAIR, DEPTH1, DEPTH2, CRPS, INSIDE, SLOTS = 0, 1, 9, 18, 19, 26, 27, 28, 29, 32
COUNT_SLOTS = [N_] + list(range(BELOW, BELOW + MAX_Q)) + list(range(PIT, PIT + MAX_Q + 1)) + [CROSS_ROWS] \
    + list(range(PAIR, PAIR + MAX_Q - 1)) + [INSIDE]
FLOAT_SLOTS = [DEPTH1, DEPTH2, CRPS]
SV_N, SV_CRPS, SV_CROSS, SV_INSIDE = 0, 1, 2, 3          # the four values per site and per time

# the kernel's own constants (csrc/grid_reduce.h, csrc/quantile_diag.hip; pinned by the CPU test against the sources)
SITES_PER_WG = 256          # GS_T
TILE_SLICES = 16            # QD_TT


def load_unroll(Q):
    """QD_U: slices whose loads are issued together."""
    return 8 if Q <= 4 else 4


def kernel_shapes(Q):
    """(the S values, the nT values) named from the kernel's constants."""
    W, TT, U = SITES_PER_WG, TILE_SLICES, load_unroll(Q)
    return [1, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1], [1, U - 1, U, U + 1, TT - 1, TT, TT + 1, 2 * TT + 1]


def levels(Q):
    """Q quantile levels as the device takes them: float32."""
    return ((np.arange(Q) + 1.0) / (Q + 1.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
def _terms(y_pred, z, split, taus, lo, hi, below=np.less_equal, crosses=np.greater):
    """Per-entry predicates and terms of the contract: everything (T, S) or (T, S, .)."""
    z = np.asarray(z)
    T, S = z.shape
    p = np.asarray(y_pred).reshape(T, S, -1).astype(np.float64)
    Q = p.shape[2]
    assert 1 <= Q <= MAX_Q
    fin = np.isfinite(z)
    zd = np.where(fin, z, 0).astype(np.float64)[:, :, None]
    code = np.zeros((T, S), dtype=np.uint8) if split is None else np.asarray(split)
    tau = np.full(Q, 0.5) if taus is None else np.asarray(taus).astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = zd - p
        rho = np.maximum((tau - 1.0) * e, tau * e)
        ck = rho[:, :, 0]
        for q in range(1, Q):
            ck = ck + rho[:, :, q]                           # left to right
        crps = (2.0 / Q) * ck
        gap = p[:, :, :-1] - p[:, :, 1:]
        depth = np.maximum(0.0, gap)
        pair = crosses(p[:, :, :-1], p[:, :, 1:])
        inside = (p[:, :, lo] <= zd[:, :, 0]) & (zd[:, :, 0] <= p[:, :, hi]) if lo >= 0 else np.zeros((T, S), bool)
    return dict(Q=Q, fin=fin, code=code, crps=crps, depth=depth, depth2=depth * depth, pair=pair,
                cross=pair.any(axis=2), below=below(zd, p), rank=(p < zd).sum(axis=2), inside=inside)


def _fsum_axis(a, axis):
    """Exact sums of a 2-D array along `axis`, correctly rounded."""
    a = a if axis == 1 else a.T
    return np.array([math.fsum(row) for row in a.tolist()])


def restate(y_pred, z, split=None, taus=None, lo=-1, hi=-1, **predicates):
    """(split_acc (4, SLOTS), site_acc (4, S, 4), time_acc (4, T, 4)) of y_pred (T*S, Q) or (T, S, Q), z (T, S) and
    split (T, S) codes or None, from zero accumulators."""
    t = _terms(y_pred, z, split, taus, lo, hi, **predicates)
    T, S = t["fin"].shape
    Q = t["Q"]
    split_acc, site_acc, time_acc = np.zeros((4, SLOTS)), np.zeros((4, S, 4)), np.zeros((4, T, 4))
    for c in range(4):
        m = t["fin"] & (t["code"] == c)
        crps = np.where(m, t["crps"], 0.0)
        for acc, ax in ((site_acc, 0), (time_acc, 1)):
            acc[c, :, SV_N] = m.sum(axis=ax)
            acc[c, :, SV_CRPS] = _fsum_axis(crps, ax)
            acc[c, :, SV_CROSS] = (m & t["cross"]).sum(axis=ax)
            acc[c, :, SV_INSIDE] = (m & t["inside"]).sum(axis=ax)
        row = split_acc[c]
        row[N_], row[CROSS_ROWS], row[INSIDE] = m.sum(), (m & t["cross"]).sum(), (m & t["inside"]).sum()
        row[BELOW:BELOW + Q] = (t["below"] & m[:, :, None]).sum(axis=(0, 1))
        row[PIT:PIT + Q + 1] = np.bincount(t["rank"][m], minlength=Q + 1)
        row[PAIR:PAIR + Q - 1] = (t["pair"] & m[:, :, None]).sum(axis=(0, 1))
        row[CRPS] = math.fsum(crps.ravel().tolist())
        row[DEPTH1] = math.fsum(t["depth"][m].ravel().tolist())
        row[DEPTH2] = math.fsum(t["depth2"][m].ravel().tolist())
    return split_acc, site_acc, time_acc


def bounds(y_pred, z, split=None, taus=None, lo=-1, hi=-1, start=None):
    """The derived bound (n + 3) 2^-53 sum|term| of every float sum: (split (4, SLOTS) -- 0 at the count slots --,
    site (4, S), time (4, T)), the last two for the crps value.  `start` = (split_acc, site_acc) before the call: the
    value already there is one more term of the sum (n + 1 terms, its magnitude in the sum of magnitudes)."""
    t = _terms(y_pred, z, split, taus, lo, hi)
    T, S = t["fin"].shape
    Q = t["Q"]
    u = 2.0 ** -53
    s_split, s_site = (np.zeros((4, SLOTS)), np.zeros((4, S, 4))) if start is None else (np.abs(start[0]), np.abs(start[1]))
    more = 0 if start is None else 1
    bs, bsite, btime = np.zeros((4, SLOTS)), np.zeros((4, S)), np.zeros((4, T))
    for c in range(4):
        m = t["fin"] & (t["code"] == c)
        a = np.where(m, np.abs(t["crps"]), 0.0)
        bsite[c] = (m.sum(axis=0) + more + 3) * u * (a.sum(axis=0) + s_site[c, :, SV_CRPS])
        btime[c] = (m.sum(axis=1) + 3) * u * a.sum(axis=1)
        bs[c, CRPS] = (m.sum() + more + 3) * u * (a.sum() + s_split[c, CRPS])
        bs[c, DEPTH1] = (m.sum() * (Q - 1) + more + 3) * u * (t["depth"][m].sum() + s_split[c, DEPTH1])
        bs[c, DEPTH2] = (m.sum() * (Q - 1) + more + 3) * u * (t["depth2"][m].sum() + s_split[c, DEPTH2])
    return bs, bsite, btime


def compare(got, ref, bound, start=None):
    """The comparator: `got`, `ref` (split_acc, site_acc, time_acc) -- an array of `got` may be None when the call
    skipped it --, `bound` from bounds(); `start` the accumulators' values before the call (None = zeros; time_acc is
    assigned, so it has none).  Every count EXACT, every float sum within its bound, every slot compared.  Returns the
    list of failures, empty when the two agree."""
    bad = []
    s0 = (0.0, 0.0) if start is None else start
    if got[0] is None or got[0].shape != ref[0].shape:
        return ["split_acc missing or misshapen"]
    d = np.abs(got[0] - (ref[0] + s0[0]))
    for c in range(4):
        for k in range(SLOTS):
            tol = bound[0][c, k] if k in FLOAT_SLOTS else 0.0
            if not d[c, k] <= tol:
                bad.append(f"split {c} slot {k}: {got[0][c, k]!r} vs {(ref[0] + s0[0])[c, k]!r} (bound {tol:.3e})")
    for name, g, r, b, st in (("site", got[1], ref[1], bound[1], s0[1]), ("time", got[2], ref[2], bound[2], 0.0)):
        if g is None:
            continue
        if g.shape != r.shape:
            bad.append(f"{name}_acc misshapen")
            continue
        dd = np.abs(g - (r + st))
        tol = np.zeros(r.shape)
        tol[:, :, SV_CRPS] = b
        for c, i, v in zip(*np.nonzero(~(dd <= tol))):
            bad.append(f"{name} split {c} index {i} value {v}: {g[c, i, v]!r} vs {(r + st)[c, i, v]!r} "
                       f"(bound {tol[c, i, v]:.3e})")
    return bad


# ------------------------------------------------------------------------------------------------ the case generator
R_SORTED, R_ONE_CROSS, R_REVERSED, R_EQUAL, R_RANDOM = range(5)
Z_RANDOM, Z_ON_LEVEL, Z_NAN, Z_PINF, Z_NINF = range(5)


def _mandatory(Q):
    """(code, row kind, pair, z kind) of the entries every case of at least 64 entries holds."""
    out = []
    for c in range(4):
        out.append((c, R_SORTED, 0, Z_RANDOM))
        for j in range(max(Q - 1, 0)):
            out.append((c, R_ONE_CROSS, j, Z_RANDOM))
        out.append((c, R_REVERSED, 0, Z_RANDOM))
        out.append((c, R_EQUAL, c % max(Q - 1, 1), Z_RANDOM))
        out.append((c, R_SORTED, 0, Z_ON_LEVEL))
        out += [(c, R_RANDOM, 0, zk) for zk in (Z_NAN, Z_PINF, Z_NINF)]
    out.append((7, R_SORTED, 0, Z_RANDOM))
    assert len(out) <= 64
    return out


def make_case(S, nT, Q, seed=0):
    """(y_pred (nT*S, Q) float32, z (nT, S) float32, split (nT, S) uint8): the mandatory entries at seeded places, the
    rest drawn -- row kind, split code (7 now and then) and z kind (about a tenth non-finite, a fifth on a level).
    Rows are multiples of 1/8 in [-12, 8]: strictly ascending steps of 1/8 .. 1, then made what their kind says."""
    rs = np.random.RandomState(1000003 * seed + 1009 * S + 31 * nT + Q)
    n = S * nT
    plan = np.array(_mandatory(Q) if n >= 64 else [], dtype=np.int64).reshape(-1, 4)
    k = n - len(plan)
    u = rs.uniform(size=k)
    zk = np.select([u < 0.04, u < 0.07, u < 0.1, u < 0.3], [Z_NAN, Z_PINF, Z_NINF, Z_ON_LEVEL], Z_RANDOM)
    drawn = np.stack([np.where(rs.uniform(size=k) < 0.05, 7, rs.randint(0, 4, size=k)), rs.randint(0, 5, size=k),
                      rs.randint(0, max(Q - 1, 1), size=k), zk], axis=1)
    plan = np.concatenate([plan, drawn])[np.argsort(rs.permutation(n))]      # the mandatory entries land anywhere
    code, rk, j, zk = plan.T
    j = np.minimum(j, max(Q - 2, 0))
    inc = rs.randint(1, 9, size=(n, Q)) / 8.0
    y = np.cumsum(inc, axis=1) - inc[:, :1] + rs.randint(-32, 8, size=(n, 1)) / 8.0
    rnd = rs.randint(-32, 33, size=(n, Q)) / 8.0
    y[rk == R_RANDOM] = rnd[rk == R_RANDOM]
    y[rk == R_REVERSED] = y[rk == R_REVERSED, ::-1]
    if Q >= 2:
        i = np.nonzero(rk == R_ONE_CROSS)[0]
        y[i, j[i]], y[i, j[i] + 1] = y[i, j[i] + 1], y[i, j[i]]
        i = np.nonzero(rk == R_EQUAL)[0]
        y[i, j[i] + 1] = y[i, j[i]]
    z = rs.randint(-80, 81, size=n) / 16.0
    on = y[np.arange(n), rs.randint(0, Q, size=n)]
    z = np.select([zk == Z_ON_LEVEL, zk == Z_NAN, zk == Z_PINF, zk == Z_NINF], [on, np.nan, np.inf, -np.inf], z)
    assert np.array_equal(y * 8, np.round(y * 8))
    return y.astype(np.float32), z.astype(np.float32).reshape(nT, S), code.astype(np.uint8).reshape(nT, S)


def conditions(y_pred, z, split):
    """What a case holds, read back from its arrays: {split code: set of condition names}."""
    T, S = z.shape
    p = y_pred.reshape(T, S, -1).astype(np.float64)
    Q = p.shape[2]
    d = np.diff(p, axis=2)
    fin = np.isfinite(z)
    out = {}
    for c in sorted(set(np.unique(split).tolist())):
        m = split == c
        have = set()
        if (m & fin & (d > 0).all(axis=2)).any():
            have.add("sorted")
        for j in range(Q - 1):
            only_j = (d[:, :, j] < 0) & ((d < 0).sum(axis=2) == 1)
            if (m & fin & only_j).any():
                have.add(f"one crossing at pair {j}")
        if Q >= 2 and (m & fin & (d < 0).all(axis=2)).any():
            have.add("reversed")
        if Q >= 2 and (m & fin & (d == 0).any(axis=2) & ~(d < 0).any(axis=2)).any():
            have.add("equal neighbours")
        if (m & fin & (p == z.astype(np.float64)[:, :, None]).any(axis=2)).any():
            have.add("z on a level")
        for name, sel in (("nan", np.isnan(z)), ("+inf", z == np.inf), ("-inf", z == -np.inf)):
            if (m & sel).any():
                have.add(name)
        out[c] = have
    return out


def required(Q):
    need = {"sorted", "z on a level", "nan", "+inf", "-inf"}
    if Q >= 2:
        need |= {"reversed", "equal neighbours"} | {f"one crossing at pair {j}" for j in range(Q - 1)}
    return need


def toggles(i_s, i_t, Q):
    """(interval, split given, site_acc given, time_acc given) of the kernel test at shape indices (i_s, i_t): the four
    bits of a number that runs through 0..15 along S, along nT and along Q."""
    h = (i_s + 3 * i_t + 5 * Q) % 16
    return bool(h & 1) and Q >= 2, bool(h & 2), bool(h & 4), bool(h & 8)


# ------------------------------------------------------------------------------------------------ end to end
E2E_S, E2E_T, E2E_SEED = 70, 19, 5
E2E_LEVELS = [0.05, 0.25, 0.5, 0.75, 0.95]
E2E_INTERVAL = (0.05, 0.95)


# the three routes of Predictor._grid_chunks: the window kernels take a first width of 128 or 256 only, and the fused tail
# refuses widths that are no multiple of 16, so the model's siblings differ from it in `hidden` alone
ROUTES = {"window": dict(hidden=(128, 16), force_window=True), "materialising": dict(hidden=(32, 16), force_window=False),
          "expanded": dict(hidden=(40, 24), force_window=False)}


def e2e_model(hidden=(32, 16), delta=False, seed=E2E_SEED):
    """A freshly initialised 5-quantile model (torch.manual_seed(seed)): [25] spatial knots, hidden [32, 16] (other
    `hidden`: its siblings of ROUTES).  `delta`: the delta head, whose
    quantile k + 1 is quantile k plus delta_k+1 . [1, h] with h >= 0 (the trunk ends in a ReLU): monotone where the
    delta vectors past the first are non-negative -- the state P_nc(delta) = 0 that the parameter-level penalty trains
    towards, which a fresh N(0, 0.01) draw is not in.  So they are made non-negative here, with an intercept of at least
    0.05 that no fp32 rounding of the two dot products can outweigh."""
    import torch
    from stnf.models import STInterpMLP
    torch.manual_seed(seed)
    m = STInterpMLP(p=0, k_spatial_centers=[25], k_temporal_centers=[10], hidden_dims=list(hidden), dropout=0.0,
                    layernorm=True, output_dim=len(E2E_LEVELS), use_delta_reparameterization=delta)
    if delta:
        with torch.no_grad():
            for d in list(m.delta_params)[1:]:
                d.abs_()
                d[0] += 0.05
    return m.eval()


def e2e_field(seed=77, S=E2E_S, T=E2E_T):
    """coords (S, 2), z (T, S) float32 with about 15 % NaN, a +inf and a -inf, split codes 0..3 (uint8)."""
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
