"""Conformal calibration (stdadk_conformal_scores_f32, stdadk_select_f32, stnf.calibration, Predictor.conformal_grid,
grid_scores' `conformal` entry, Evaluator's `conformal`): the case generators, the comparators of the GPU test and the
end-to-end model.  Shared by tests/test_conformal_cases_cpu.py (runs anywhere) and tests/test_gpu_conformal.py.  Not
imported by the product.  The references are numpy's own: float32 arithmetic and boolean-mask order for the scores,
np.sort for the order statistics.

SCORE CASES.  `make_score_case(S, nT, Q, seed)` -> y_pred (nT*S, Q), z (nT, S), code (nT, S): predictions and values
are unrounded float32 draws (the scores must match numpy to the bit, so nothing is made exactly representable); codes
are drawn from {0, 1, 2, 3, 7}; z has NaN, +inf and -inf holes once there are entries enough; with nT >= 3 time slice 1
has no member of either segment (code 7 throughout) and time slice nT - 1 is all members of segment 0 (code 2, finite
z); with three runs of the kernel's 1 024 rows or more, run 1 has no member and run 2 is all members.
`conditions()` reads the promises back from the arrays.

KEY CASES.  `make_keys(family, n, seed)` -> n finite float32 values of one of FAMILIES.
"""
import numpy as np

RESID, CQR, ABS = 0, 1, 2
MAX_COLS, MAX_SEGMENTS, MAX_SELECT = 8, 2, 16
RUN = 1024                                   # CS_RUN of csrc/conformal.hip: rows per run of the compaction
SELECT_BITS = 8                              # SEL_BITS

SCORE_S = [1, 63, 64, 65, 255, 256, 257, 513]
SCORE_T = [1, 3, 4, 5, 16, 17, 33]
SCORE_Q = [1, 3, 5, 8]
CODE_POOL = [0, 1, 2, 3, 7]
SEGMENT_CODES = [2, 3]                       # calibration, evaluation

KEY_N = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65537, 1048579]
SMALL_N = 257                                # every rank is tried up to here
FAMILIES = ["uniform", "equal", "two", "seven", "low_byte", "top_byte", "zeros", "denormal", "fltmax"]
FLT_MAX = np.finfo(np.float32).max


def score_cols(Q):
    """The score columns of a case: RESID of up to six levels, CQR of the outer pair, ABS of the median."""
    return [(RESID, q, 0) for q in range(min(Q, 6))] + [(CQR, 0, Q - 1), (ABS, Q // 2, 0)]


def make_score_case(S, nT, Q, seed=0):
    rs = np.random.RandomState(1000 * seed + 97 * S + 13 * nT + Q)
    y = (0.7 * rs.standard_normal((nT * S, Q))).astype(np.float32)
    z = (0.9 * rs.standard_normal((nT, S))).astype(np.float32)
    code = np.asarray(CODE_POOL, dtype=np.uint8)[rs.randint(0, len(CODE_POOL), size=(nT, S))]
    n = nT * S
    cf, zf = code.reshape(-1), z.reshape(-1)
    free = np.ones(n, dtype=bool)              # where a hole may go: not in a slice or run that is all members
    if nT >= 3:
        code[1] = 7
        code[nT - 1] = SEGMENT_CODES[0]
        free[(nT - 1) * S:] = False
    if n >= 3 * RUN:
        cf[RUN:2 * RUN] = 7
        cf[2 * RUN:3 * RUN] = SEGMENT_CODES[0]
        free[2 * RUN:3 * RUN] = False
    if n >= 8:
        spots = np.flatnonzero(free)
        holes = spots[rs.choice(spots.size, size=max(3, spots.size // 9), replace=False)]
        zf[holes] = np.nan
        zf[holes[0]], zf[holes[1]] = np.inf, -np.inf
    return y, z, code


def conditions(y, z, code):
    """What a case holds, read from the arrays."""
    nT, S = z.shape
    n = nT * S
    member = np.isfinite(z)[None] & (code[None] == np.asarray(SEGMENT_CODES)[:, None, None])      # (G, nT, S)
    flat = member.reshape(len(SEGMENT_CODES), -1)
    runs = [flat[:, r:r + RUN] for r in range(0, n - n % RUN, RUN)]
    return {"nan": bool(np.isnan(z).any()), "pinf": bool(np.isposinf(z).any()), "ninf": bool(np.isneginf(z).any()),
            "other_code": bool((code == 7).any()),
            "empty_slice": bool((~member.any(axis=(0, 2))).any()),
            "full_slice": bool(member[0].all(axis=1).any()),
            "empty_run": any(not r.any() for r in runs), "full_run": any(r[0].all() for r in runs),
            "members": flat.sum(axis=1)}


def promised(S, nT):
    """The keys of conditions() a case of this shape must hold true."""
    n = S * nT
    out = []
    if n >= 8:
        out += ["nan", "pinf", "ninf"]
    if nT >= 3:
        out += ["empty_slice", "full_slice", "other_code"]
    if n >= 3 * RUN:
        out += ["empty_run", "full_run"]
    return out


def make_keys(family, n, seed=0):
    rs = np.random.RandomState(7919 * seed + 31 * FAMILIES.index(family) + n % 1009)
    f32 = lambda bits: np.asarray(bits, dtype=np.uint32).view(np.float32)      # noqa: E731
    if family == "uniform":
        x = rs.uniform(-1.0, 1.0, n)
    elif family == "equal":
        x = np.full(n, 0.37)
    elif family == "two":
        x = np.asarray([-1.5, 2.25])[rs.randint(0, 2, n)]
    elif family == "seven":
        x = np.asarray([-3.0, -0.125, 0.0, 0.5, 0.75, 2.0, 1.0e3])[rs.randint(0, 7, n)]
    elif family == "low_byte":
        x = f32(0x3F800000 | rs.randint(0, 256, n).astype(np.uint32))
    elif family == "top_byte":
        x = f32((rs.randint(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456))
    elif family == "zeros":
        x = np.asarray([0.0, -0.0, 1.0e-3, -1.0e-3], dtype=np.float32)[rs.randint(0, 4, n)]
    elif family == "denormal":
        x = f32(rs.randint(1, 0x800000, n).astype(np.uint32) | (rs.randint(0, 2, n).astype(np.uint32) << np.uint32(31)))
    elif family == "fltmax":
        x = np.asarray([FLT_MAX, -FLT_MAX, 0.0, 1.0], dtype=np.float32)[rs.randint(0, 4, n)]
    else:
        raise KeyError(family)
    return np.ascontiguousarray(x, dtype=np.float32)


def ranks(n):
    """Every rank up to SMALL_N values, else {0, 1, n/2, n - 2, n - 1}."""
    return list(range(n)) if n <= SMALL_N else sorted({0, 1, n // 2, n - 2, n - 1})


# ------------------------------------------------------------------------------------------------ the comparators
def compare_select(x, rank, value, rank_used, ordered=None):
    """[] when (value, rank_used) is the rank-th smallest of x (0-based, by value: -0 == +0) and the rank itself, or
    (+inf, -1) for a rank outside 0..n-1; else what is wrong.  `ordered`: np.sort(x), when the caller has it."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    bad = []
    if rank < 0 or rank >= x.size:
        if not (np.isposinf(value) and rank_used == -1):
            bad.append(("beyond", int(rank), float(value), int(rank_used)))
        return bad
    want = (np.sort(x) if ordered is None else ordered)[rank]
    if not (np.float32(value) == want):
        bad.append(("value", int(rank), float(value), float(want)))
    if int(rank_used) != int(rank):
        bad.append(("rank_used", int(rank), int(rank_used)))
    return bad


def compare_segments(scores, count, ref, cap=None):
    """[] when segment g of scores (G, C, cap) holds ref[g] (C, n_g) from index 0 on, bit for bit, and count[g] == n_g
    (with `cap` below n_g: the first cap scores, count == cap); else what is wrong."""
    bad = []
    for g, want in enumerate(ref):
        n = want.shape[1] if cap is None else min(want.shape[1], cap)
        if int(count[g]) != n:
            bad.append(("count", g, int(count[g]), n))
            continue
        got = np.ascontiguousarray(scores[g][:, :n], dtype=np.float32)
        if not np.array_equal(got.view(np.uint32), np.ascontiguousarray(want[:, :n]).view(np.uint32)):
            bad.append(("bits", g, int((got.view(np.uint32) != np.ascontiguousarray(want[:, :n]).view(np.uint32)).sum())))
    return bad


# ------------------------------------------------------------------------------------------------ end to end
E2E_S, E2E_T, E2E_SEED = 70, 9, 11
E2E_LEVELS = [0.1, 0.5, 0.9]
E2E_INTERVAL = (0.1, 0.9)
E2E_ALPHA = 0.2
E2E_MAX_ROWS = 3 * E2E_S + 5                 # three slices per chunk: three chunks


def e2e_model(seed=E2E_SEED, quantiles=True):
    """A freshly initialised tiny model: [9] spatial and [5] temporal knots, hidden [32, 16]; three quantiles or one
    output (the mean model)."""
    import torch
    from stnf.models import STInterpMLP
    torch.manual_seed(seed)
    return STInterpMLP(p=0, k_spatial_centers=[9], k_temporal_centers=[5], hidden_dims=[32, 16], dropout=0.0,
                       layernorm=True, output_dim=len(E2E_LEVELS) if quantiles else 1).eval()


def e2e_field(seed=78, S=E2E_S, T=E2E_T):
    """coords (S, 2), z (T, S) float32 with about 10 % NaN, split codes 0..3 (uint8)."""
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = (0.3 * rs.standard_normal((T, S))).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.10] = np.nan
    code = rs.randint(0, 4, size=(T, S)).astype(np.uint8)
    return coords, z, code


def grid_times(T):
    return (np.arange(T, dtype=np.float32) / np.float32(T - 1)) if T > 1 else np.zeros(1, dtype=np.float32)
