"""Neighbour tables (stdadk_knn_f32, stdadk_knn_apply_f32, stnf.utils.baselines): the case generator, the tests' own
restatement and the comparators.  Shared by tests/test_knn_cases_cpu.py (runs anywhere) and tests/test_gpu_knn.py.  Not
imported by the product; no stored arrays.

CONTRACT (include/stdadk.h), restated.  d2 = dx dx + dy dy in float64 from the float32 operands, every operation rounded
once; a NaN d2 is never a neighbour.  The neighbours of a target are the k smallest sources of its slice in the TOTAL
order (d2, source index), in that order, a short row ending in idx = -1, d2 = +inf.  A table applied to a field:
nearest = z at the first entry; idw = the mean of z over the leading run of zero distances, or sum(w z) / sum(w) with
w = d^-power, sequentially in row order in double, rounded to float32 once.

COMPARISON.  The table and both outputs of the apply are compared for EQUALITY of bits (NaN positions included): the
order is total and every operation is a correctly rounded IEEE operation any restatement repeats.  The independent
restatement (restate_search) is a python loop that sorts (d2, index) tuples with d2 in np.longdouble, formed from
differences it asserts to be EXACT; the d2 it reports is the contract's float64 value from python floats, one pair at
a time, asserted to be the longdouble value rounded (within 2^-52 relative).  Two sources whose longdouble d2 differ but
round to the same float64 would be ordered by index in the contract and by value in the restatement; on the lattice
every d2 is exact in both, and the random cases hold no such pair (the comparison would show it).
The idw value is also held against np.longdouble sums within 0.5 ulp_f32 + (k + 4) 2^-52 sum(w |z|) / sum(w): k
products and k sums in each of num and den, the weight's own three operations and the quotient, first order.
"""
import math

import numpy as np

# the constants of csrc/knn.hip (pinned by the CPU test against the source)
WAVES = 4                                       # KN_Q
TILE_M = 64                                     # KN_MT: targets per workgroup
CHUNK_S = 256                                   # KN_SC: sources staged per chunk
QUARTER_S = CHUNK_S // WAVES                    # KN_SQ: a wave's share of a chunk
FILL = 1024                                     # KN_FILL: workgroups below which the sources are cut
MAX_SPANS = 64                                  # KN_MAX_SPANS
MAX_K = 16

SIZES_M = [1, 63, 64, 65, 130]                  # lane and tile edges
SIZES_S = [0, 1, 15, 16, 17, 255, 256, 257, 1025]      # list-fill, quarter and chunk edges
SIZES_K = [1, 2, 7, 8, 16]
SLICES = [1, 3]
KINDS = ("uniform", "clustered", "lattice")
POWERS = (0, 1, 2, 3, 4)


def spans(M, S, nM):
    """(G, sources per span): the launch plan's span rule, restated from the head comment of csrc/knn.hip."""
    chunks = -(-S // CHUNK_S)
    if chunks == 0 or M == 0 or nM == 0:
        return 0, CHUNK_S
    want = min(-(-FILL // (-(-M // TILE_M) * nM)), MAX_SPANS, chunks)
    per = -(-chunks // want)
    return -(-chunks // per), per * CHUNK_S


def points(rs, n, kind):
    """n float32 points: uniform in the unit square; clustered (five tight clusters); or a LATTICE of spacing 1/4 with
    repeated points, where equal and zero distances are the rule."""
    if kind == "uniform":
        return rs.uniform(0, 1, (n, 2)).astype(np.float32)
    if kind == "clustered":
        centres = rs.uniform(0.1, 0.9, (5, 2))
        return (centres[rs.randint(5, size=n)] + 0.01 * rs.standard_normal((n, 2))).astype(np.float32)
    return (rs.randint(0, 5, (n, 2)) / 4.0).astype(np.float32)


def make_case(M, S, k, nM, kind="uniform", density=1.0, exclude_self=False, nan=False, seed=0):
    """One case as a dict: q (M, 2), coords (S, 2) float32, src (nM, S) uint8 or None, k, exclude_self, z (nT, S) float32
    (nT = nM, or 3 for a shared table).  density 1.0 with nM == 1 passes src = None (every site); otherwise each site is
    a source of a slice with that probability, the LAST slice of several has none at all.  exclude_self: the targets ARE
    the sources (M = S).  nan: a NaN coordinate in source 0 and in target 0 (and an inf in source 1 where there is one)."""
    rs = np.random.RandomState(7919 * seed + 131 * M + 17 * S + 3 * k + nM + 1000 * KINDS.index(kind))
    coords = points(rs, S, kind)
    q = coords.copy() if exclude_self else points(rs, M, kind)
    if not exclude_self and kind == "uniform" and S:
        q[::5] = coords[rs.randint(S, size=len(q[::5]))]      # every fifth target ON a source: d2 = 0
    if nan:
        if S:
            coords[0, 0] = np.nan
        if S > 1:
            coords[1, 1] = np.inf
        if exclude_self:
            q = coords.copy()
        elif len(q):
            q[0, 1] = np.nan
    src = None
    if density < 1.0 or nM > 1:
        src = (rs.uniform(size=(nM, S)) < density).astype(np.uint8)
        src[src != 0] = rs.randint(1, 256, size=int((src != 0).sum()))      # any non-zero byte is a source
        if nM > 1:
            src[-1] = 0
    nT = nM if nM > 1 else 3
    z = rs.standard_normal((nT, S)).astype(np.float32)
    if S > 3:
        z[0, 3] = np.nan                        # a non-finite value at a source propagates
    return dict(q=q, coords=coords, src=src, k=k, exclude_self=exclude_self, z=z)


def all_cases():
    """Every M against 257 sources (one tile is cut into two spans there), every S against 65 targets, every k and both
    slice counts in turn, the three kinds of coordinates in turn; then the densities down to fewer than k sources,
    leave-one-out on each kind, NaN coordinates, and the span seam."""
    out = []
    n = 0
    for M in SIZES_M:
        out.append(make_case(M, 257, SIZES_K[n % 5], SLICES[n % 2], KINDS[n % 3], seed=n))
        n += 1
    for S in SIZES_S:
        out.append(make_case(65, S, SIZES_K[n % 5], SLICES[n % 2], KINDS[n % 3], seed=n))
        n += 1
    for k in SIZES_K:                            # every list size on the lattice: ties everywhere, merged over four waves
        out.append(make_case(130, 300, k, 1, "lattice", seed=n))
        n += 1
    for density in (0.5, 0.02, 0.0):             # down to fewer than k sources and to none
        out.append(make_case(65, 257, 8, 3, "uniform", density=density, seed=n))
        n += 1
    for kind in KINDS:                           # targets equal to the sources, leave-one-site-out
        out.append(make_case(0, 130, 7, 3, kind, density=0.6, exclude_self=True, seed=n))
        out.append(make_case(0, 17, 16, 1, kind, exclude_self=True, seed=n + 1))
        n += 2
    out.append(make_case(65, 40, 8, 1, "uniform", nan=True, seed=n))
    out.append(make_case(0, 40, 2, 3, "lattice", density=0.7, exclude_self=True, nan=True, seed=n + 1))
    out.append(span_seam_case())
    return out


def span_seam_case():
    """The smallest sizes at which the plan uses more than one span: one tile of one slice and S = CHUNK_S + 1 (two
    spans of one chunk, the second holding ONE source), on the lattice so that ties cross the seam; and with it the
    largest case of the suite: 1025 sources in five spans for one tile."""
    assert spans(TILE_M, CHUNK_S, 1)[0] == 1 and spans(TILE_M, CHUNK_S + 1, 1)[0] == 2
    return make_case(TILE_M, 1025, 16, 1, "lattice", seed=99)


def make_raster_case(n_sites, ny, nx):
    """n_sites random float32 sites, a value per site, against ny x nx nodes (RandomState(20261021))."""
    rs = np.random.RandomState(20261021)
    coords = rs.uniform(0, 1, (n_sites, 2)).astype(np.float32)
    values = rs.standard_normal(n_sites).astype(np.float32)
    return dict(coords=coords, values=values, ny=ny, nx=nx)


RASTER_CASES = ((300, 200, 200), (997, 37, 41))


# ---- the independent restatement ---------------------------------------------------------------

def restate_search(case):
    """The table by python loops: per (slice, target) the sources' (d2, index) tuples with d2 in np.longdouble from
    differences asserted exact, sorted with `sorted`, the first k kept; d2 is reported as the contract's float64 value
    (python floats, every operation rounded once), asserted to be the longdouble value rounded."""
    q, c, src, k = case["q"], case["coords"], case["src"], case["k"]
    M, S = len(q), len(c)
    nM = 1 if src is None else len(src)
    idx = np.full((nM, M, k), -1, dtype=np.int32)
    d2 = np.full((nM, M, k), np.inf)
    L = np.longdouble
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    qL, cL = q.astype(L), c.astype(L)
    for j in range(M):
        with np.errstate(invalid="ignore", over="ignore"):
            dL = qL[j][None, :] - cL                                         # (S, 2) longdouble
            d2L = dL[:, 0] * dL[:, 0] + dL[:, 1] * dL[:, 1]
            d = q64[j][None, :] - c64                                        # float64, every operation rounded once
            d2f = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        fin = np.isfinite(d2f)
        assert np.array_equal(np.isnan(d2f), np.isnan(d2L)) and np.array_equal(fin, np.isfinite(d2L))
        assert (d.astype(L)[fin] == dL[fin]).all(), "a difference that is not exact in float64"
        assert (np.abs(d2f.astype(L)[fin] - d2L[fin]) <= L(2.0 ** -52) * d2L[fin]).all()
        d2L_list, d2f_list = list(d2L), d2f.tolist()
        for m in range(nM):
            sel = range(S) if src is None else np.nonzero(src[m])[0].tolist()
            cand = [(d2L_list[i], i, d2f_list[i]) for i in sel
                    if not (case["exclude_self"] and i == j) and not math.isnan(d2f_list[i])]
            for e, (_, i, dd) in enumerate(sorted(cand)[:k]):
                idx[m, j, e], d2[m, j, e] = i, dd
    return idx, d2


def restate_apply(idx, d2, k, z, power):
    """nearest and the idw value in np.longdouble, with the terms for the bound: returns nearest (nT, M) float32, idw
    (nT, M) longdouble, and scale (nT, M) longdouble = sum(w |z|) / sum(w) (|mean| terms for the zero branch)."""
    nM, M, _ = idx.shape
    nT, S = z.shape
    nearest = np.full((nT, M), np.nan, dtype=np.float32)
    idw = np.full((nT, M), np.nan, dtype=np.longdouble)
    scale = np.zeros((nT, M), dtype=np.longdouble)
    L = np.longdouble
    for ti in range(nT):
        m = 0 if nM == 1 else ti
        for j in range(M):
            ent = [(int(i), float(d)) for i, d in zip(idx[m, j, :k], d2[m, j, :k]) if 0 <= i < S]
            if not ent:
                continue
            nearest[ti, j] = z[ti, ent[0][0]]
            if ent[0][1] == 0.0:
                run = []
                for i, d in ent:
                    if d != 0.0:
                        break
                    run.append(L(z[ti, i]))
                idw[ti, j] = sum(run, L(0)) / L(len(run))
                scale[ti, j] = sum((abs(v) for v in run), L(0)) / L(len(run))
                continue
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                w = [L(1) if power == 0 else L(1) / (np.sqrt(L(d)) ** power) for _, d in ent]
                num = sum((wi * L(z[ti, i]) for wi, (i, _) in zip(w, ent)), L(0))
                den = sum(w, L(0))
                idw[ti, j] = num / den
                scale[ti, j] = sum((wi * abs(L(z[ti, i])) for wi, (i, _) in zip(w, ent)), L(0)) / den
    return nearest, idw, scale


def same_bits(a, b):
    """Equal shapes, dtypes and bits, every NaN matching a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(np.array_equal(np.isnan(a), np.isnan(b))) and \
            bool(np.array_equal(np.where(np.isnan(a), 0, a).view(f"u{a.itemsize}"), np.where(np.isnan(b), 0, b).view(f"u{b.itemsize}")))
    return bool(np.array_equal(a, b))


def same_table(got_idx, got_d2, want_idx, want_d2):
    return same_bits(np.asarray(got_idx, dtype=np.int32), np.asarray(want_idx, dtype=np.int32)) and \
        same_bits(np.asarray(got_d2, dtype=np.float64), np.asarray(want_d2, dtype=np.float64))
