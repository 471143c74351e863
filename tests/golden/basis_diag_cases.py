"""Basis diagnostics (stdadk_basis_diag_f32, stdadk_group_norms_f32, Predictor.basis_diagnostics,
stnf.utils.basis_diag): the case generator, the bound, the comparator and the tests' own long-double restatement.
Shared by tests/test_basis_diag_cases_cpu.py (runs anywhere) and tests/test_gpu_basis_diag.py.  Not imported by the
product.

CONTRACT (include/stdadk.h), restated.  d2 = dx dx + dy dy in float64 from the float32 operands, every operation rounded
once; den_k = (double)bw_k cal, s_k = den_k rho, R2_k = s_k s_k; the pair (site i, knot k) is IN SUPPORT iff d2 < R2_k.
In support r = sqrt(d2) / den_k and phi(r) in double.  knot_acc [Ks][7] = (N, W, SPHI, SPHI2, SV, WV, NEAR2) over the
sites whose w is finite and > 0; site_acc [S][L][3] = (COVER, SPHI, NEAR2) for every site and level.

BOUND.  N, COVER and both NEAR2 are decided by exact comparisons of values every restatement forms with the same IEEE
operations: they are compared for EQUALITY.  Every sum is compared by

    |got - want| <= 2^-52 (n want + 64 A)

with n the slot's number of terms and A the sum of w over its terms (for a site row w = 1, so A = COVER).  Derivation:
  * adding n non-negative terms in ANY fixed order is within n 2^-52 of the exact sum, relative (at most n roundings of
    2^-53 relative each on the way of any term, first order, a factor 2 to spare): the n want part;
  * a TERM w phi(r) is not exact either.  phi <= 1 and |phi'| <= 3 for all three kinds (Wendland C4's steepest slope is
    about 2.5 at r near 0.3, the Gaussian's e^-1/2 < 1, the triangular's 1), so the term's ABSOLUTE error is at most
    w (3 dr + dphi), dr the error of r and dphi that of evaluating phi at the r it was handed.  r <= rho <= 4.5 comes
    from three rounded operations on top of d2's five (d2, sqrt, the quotient with den = bw cal, itself rounded): at most
    about 5 roundings of relative 2^-53 that reach r at full weight, dr <= 5 x 4.5 x 2^-53 = 11.25 x 2^-52; dphi is at
    most eight rounded operations on values <= 56 scaled back by the final product into [0, 1], under 8 x 2^-52 for
    the polynomial kinds, and for the Gaussian the argument's error (|arg| <= 10.2, three roundings: 15.3 x 2^-52 once
    through exp' <= 1) plus exp's own ulp.  3 dr + dphi < (34 + 17) 2^-52 w < 64 x 2^-52 w: the 64 A part.
  * a bound relative to the TERM would be wrong: near the support edge (1 - r)^6 amplifies the relative error without
    limit while the absolute error vanishes.
SV's terms carry the factor v: its n counts the in-support sites with a finite v, `want` is the sum of w phi |v| and A
the sum of w |v| over them; WV's are n, WV and the sum of w over the same sites.
The constant 64 is a condition: tests/test_basis_diag_cases_cpu.py shows the numpy float64 restatement within ONE QUARTER
of the bound of the long-double restatement below on every case, and records the worst ratio in
basis_diag_achieved.json (python tests/golden/basis_diag_cases.py rewrites it).
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ACHIEVED = os.path.join(HERE, "basis_diag_achieved.json")

K_N, K_W, K_SPHI, K_SPHI2, K_SV, K_WV, K_NEAR2 = range(7)
S_COVER, S_SPHI, S_NEAR2 = range(3)
CAL = {"wendland": 1.0, "gaussian": 0.223477, "triangular": 0.654714}
BASES = ("wendland", "gaussian", "triangular")

# the constants of csrc/basis_diag.hip (pinned by the CPU test against the source)
WAVES = 4                                       # BD_Q: waves per workgroup of either direction
TILE_K = 64                                     # BD_KT: knots per workgroup of the knot direction
CHUNK_S = 64                                    # BD_SC: a wave's sub-chunk of sites; a span is whole sub-chunks
STAGE_S = WAVES * CHUNK_S                       # BD_SS: sites staged at a time
MAX_SPANS = 16                                  # BD_MAX_SPANS
TILE_S = 64                                     # BD_ST: sites per workgroup of the site direction
CHUNK_K = 256                                   # BD_KC: knots staged per chunk of the site direction
QUARTER_K = CHUNK_K // WAVES                    # BD_KQ: a wave's share of a staged chunk of knots

# 1; below / at / above the sub-chunk and site-tile edge 64; 129 (two waves' sub-chunks and one site of a third);
# below / at / above the staged block 256; 1000 (16 spans, the last ragged); below / at / above
# MAX_SPANS x CHUNK_S = 1024, where a span becomes two sub-chunks; 1090 (nine spans of 128, the last ragged)
SIZES_S = [1, CHUNK_S - 1, CHUNK_S, CHUNK_S + 1, 2 * CHUNK_S + 1, STAGE_S - 1, STAGE_S, STAGE_S + 1, 1000,
           MAX_SPANS * CHUNK_S - 1, MAX_SPANS * CHUNK_S, MAX_SPANS * CHUNK_S + 1, 1090]
# 1; below / at / above the knot tile and a wave's quarter of a chunk, 64; 74 (the smallest table the split
# (3, 70, Ks - 73) fits); the shipped 227; below / at / above the staged chunk 256; 513 (two chunks and one knot); 600
SIZES_K = [1, TILE_K - 1, TILE_K, TILE_K + 1, 74, 227, CHUNK_K - 1, CHUNK_K, CHUNK_K + 1, 2 * CHUNK_K + 1, 600]
S_FOR_K, K_FOR_S = 2 * CHUNK_S + 1, 227


def level_splits(Ks):
    """(Ks,), the shipped (25, 81, 121) when it fits, and one that cuts inside a tile: (3, 70, Ks - 73)."""
    out = [(Ks,)]
    if Ks == 227:
        out.append((25, 81, 121))
    if Ks > 73:
        out.append((3, 70, Ks - 73))
    return out


def shapes():
    """(S, Ks, level sizes) of every case: each S against the shipped table, each Ks against 129 sites, each level
    split in turn, and the two largest together."""
    out = []
    for n, S in enumerate(SIZES_S):
        sp = level_splits(K_FOR_S)
        out.append((S, K_FOR_S, sp[n % len(sp)]))
    for n, Ks in enumerate(SIZES_K):
        sp = level_splits(Ks)
        out.append((S_FOR_K, Ks, sp[(n + 1) % len(sp)]))
    out += [(1090, 600, (3, 70, 527)), (MAX_SPANS * CHUNK_S + 1, CHUNK_K + 1, (CHUNK_K + 1,))]
    return out


def make_case(S, Ks, sizes, basis, seed=0, toggle=0):
    """One case as a dict: centers (Ks, 2), bw (Ks,), coords (S, 2) float32, w / v (S,) float64 or None, rho, sizes.
    Knots uniform in [-0.1, 1.1]^2 (some out of the domain) with bandwidths 0.05 .. 0.45; sites uniform in the unit
    square with site 1 a DUPLICATE of site 0 and every seventh site ON a knot (d2 = 0).  toggle bit 0: w given
    (counts 0 .. 5 with a negative, a NaN and an inf among them), else NULL; bit 1: v given (with NaNs), else NULL;
    bit 2: rho away from the default."""
    rs = np.random.RandomState(1009 * seed + 31 * S + Ks + 7 * BASES.index(basis))
    centers = rs.uniform(-0.1, 1.1, (Ks, 2)).astype(np.float32)
    bw = rs.uniform(0.05, 0.45, Ks).astype(np.float32)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    if S >= 2:
        coords[1] = coords[0]
    for i in range(2, S, 7):
        coords[i] = centers[rs.randint(Ks)]
    w = v = None
    if toggle & 1:
        w = rs.randint(0, 6, S).astype(np.float64)
        for i, bad in zip(rs.choice(S, min(S, 3), replace=False), (-2.0, np.nan, np.inf)):
            if S > 3:
                w[i] = bad
    if toggle & 2:
        v = rs.uniform(0, 2, S) ** 2
        v[rs.uniform(size=S) < 0.2] = np.nan
        if S > 5:
            v[5] = np.inf
    rho = 1.0 if basis != "gaussian" else 1.0 / CAL[basis]
    if toggle & 4:
        rho = {"wendland": 0.75, "gaussian": 2.5, "triangular": 1.5}[basis]
    return dict(centers=centers, bw=bw, basis=basis, sizes=tuple(sizes), coords=coords, w=w, v=v, rho=rho)


def all_cases(basis):
    """The cases of one basis kind; the toggles cycle through all eight combinations along them."""
    return [make_case(S, Ks, sizes, basis, seed=n, toggle=(n + BASES.index(basis)) % 8)
            for n, (S, Ks, sizes) in enumerate(shapes())]


def call_args(case):
    """The arguments of the restatements of stnf.utils.basis_diag for a case."""
    return (case["centers"], case["bw"], case["basis"], case["sizes"], case["coords"], case["w"], case["v"], case["rho"])


# ------------------------------------------------------------------------------------------------ the long-double side
def _pairs(case, dtype):
    """(inside (S, Ks) by the CONTRACT's float64 comparison, d2 float64, phi in `dtype` from d2 formed in `dtype`)."""
    c64 = case["centers"].astype(np.float64)
    x64 = case["coords"].astype(np.float64)
    den64 = case["bw"].astype(np.float64) * CAL[case["basis"]]
    s = den64 * case["rho"]
    dx, dy = x64[:, None, 0] - c64[None, :, 0], x64[:, None, 1] - c64[None, :, 1]
    d2 = dx * dx + dy * dy
    inside = d2 < (s * s)[None, :]
    c, x = case["centers"].astype(dtype), case["coords"].astype(dtype)
    den = case["bw"].astype(dtype) * dtype(CAL[case["basis"]])
    ex, ey = x[:, None, 0] - c[None, :, 0], x[:, None, 1] - c[None, :, 1]
    r = np.sqrt(ex * ex + ey * ey) / den[None, :]
    if case["basis"] == "wendland":
        r = np.minimum(r, dtype(1))
        om = dtype(1) - r
        phi = om ** 6 * ((dtype(35) * r + dtype(18)) * r + dtype(3)) / dtype(3)
    elif case["basis"] == "gaussian":
        phi = np.exp(dtype(-0.5) * r * r)
    else:
        phi = np.maximum(dtype(1) - r, dtype(0))
    return inside, d2, np.where(inside, phi, dtype(0))


def restate_longdouble(case):
    """The reference of the bound: the in-support decisions and the minima as the contract makes them (float64), every
    term and every sum in np.longdouble from the float32 operands.  Returns (knot (Ks, 7), site (S, L, 3)) as long
    doubles and `aux`, what the comparator needs beside them: per knot NV (the count of SV's terms), AV (their sum of
    w), AVV (of w |v|), SVABS (of w phi |v|)."""
    ld = np.longdouble
    inside, d2, phi = _pairs(case, ld)
    S, Ks = d2.shape
    sizes = case["sizes"]
    w = np.ones(S) if case["w"] is None else case["w"]
    counted = np.isfinite(w) & (w > 0)
    wc = np.where(counted, w, 0.0).astype(ld)
    v = case["v"]
    vfin = np.isfinite(v) if v is not None else np.zeros(S, dtype=bool)
    vz = (np.where(vfin, v, 0.0) if v is not None else np.zeros(S)).astype(ld)
    hit = inside & counted[:, None]
    t = wc[:, None] * phi
    hv = hit & vfin[:, None]
    knot = np.zeros((Ks, 7), dtype=ld)
    knot[:, K_N] = hit.sum(axis=0)
    knot[:, K_W] = np.where(hit, wc[:, None], ld(0)).sum(axis=0)
    knot[:, K_SPHI] = t.sum(axis=0)
    knot[:, K_SPHI2] = (t * phi).sum(axis=0)
    knot[:, K_SV] = np.where(hv, t * vz[:, None], ld(0)).sum(axis=0)
    knot[:, K_WV] = np.where(hv, t, ld(0)).sum(axis=0)
    knot[:, K_NEAR2] = np.where(counted[:, None], d2, np.inf).min(axis=0, initial=np.inf)
    aux = {"NV": hv.sum(axis=0).astype(np.float64),
           "AV": np.where(hv, wc[:, None], ld(0)).sum(axis=0).astype(np.float64),
           "AVV": np.where(hv, wc[:, None] * np.abs(vz)[:, None], ld(0)).sum(axis=0).astype(np.float64),
           "SVABS": np.where(hv, t * np.abs(vz)[:, None], ld(0)).sum(axis=0).astype(np.float64)}
    site = np.zeros((S, len(sizes), 3), dtype=ld)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for l in range(len(sizes)):
        a, b = off[l], off[l + 1]
        site[:, l, S_COVER] = inside[:, a:b].sum(axis=1)
        site[:, l, S_SPHI] = phi[:, a:b].sum(axis=1)
        site[:, l, S_NEAR2] = d2[:, a:b].min(axis=1, initial=np.inf)
    return knot, site, aux


def aux_of(case):
    return restate_longdouble(case)[2]


# ------------------------------------------------------------------------------------------------ the comparator
def bounds(ref_knot, ref_site, aux):
    """The allowed |got - want| per slot, 0 for the slots compared for equality: 2^-52 (n want + 64 A)."""
    rk, rsite = np.asarray(ref_knot, dtype=np.float64), np.asarray(ref_site, dtype=np.float64)
    u = 2.0 ** -52
    bk, bs = np.zeros(rk.shape), np.zeros(rsite.shape)
    n, W = rk[:, K_N], rk[:, K_W]
    for slot in (K_W, K_SPHI, K_SPHI2):
        bk[:, slot] = u * (n * rk[:, slot] + 64.0 * W)
    bk[:, K_SV] = u * (aux["NV"] * aux["SVABS"] + 64.0 * aux["AVV"])
    bk[:, K_WV] = u * (aux["NV"] * rk[:, K_WV] + 64.0 * aux["AV"])
    cover = rsite[:, :, S_COVER]
    bs[:, :, S_SPHI] = u * (cover * rsite[:, :, S_SPHI] + 64.0 * cover)
    return bk, bs


def compare(got_knot, got_site, ref_knot, ref_site, aux, fraction=1.0):
    """`got` against `ref`: N, COVER and both NEAR2 EXACT, every sum within `fraction` of its bound.  Returns (the list
    of failures, empty when the two agree; the worst |got - want| / bound over the sums with a positive bound)."""
    gk, gs = np.asarray(got_knot, dtype=np.longdouble), np.asarray(got_site, dtype=np.longdouble)
    rk, rs_ = np.asarray(ref_knot, dtype=np.longdouble), np.asarray(ref_site, dtype=np.longdouble)
    if gk.shape != rk.shape or gs.shape != rs_.shape:
        return [f"shapes {gk.shape}, {gs.shape} vs {rk.shape}, {rs_.shape}"], np.inf
    bk, bs = bounds(ref_knot, ref_site, aux)
    bad, worst = [], 0.0
    for name, g, r, b in (("knot", gk, rk, bk), ("site", gs, rs_, bs)):
        with np.errstate(invalid="ignore"):
            diff = np.where(g == r, np.longdouble(0), np.abs(g - r)).astype(np.float64)      # (inf - inf: equal)
        ok = diff <= fraction * b
        for idx in zip(*np.nonzero(~ok)):
            bad.append(f"{name}{list(map(int, idx))}: {float(g[idx])!r} vs {float(r[idx])!r} (bound {b[idx]:.3e})")
        pos = b > 0
        if pos.any():
            worst = max(worst, float((diff[pos] / b[pos]).max()))
    return bad, worst


# ------------------------------------------------------------------------------------------------ boundary cases
def next_below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def dyadic_boundary_case():
    """Wendland, one knot at the origin with bw = 0.25 (R2 = 1/16 exactly): sites at axis distance exactly 0.25 on both
    axes (OUT: the comparison is strict), at the next float32 below 0.25 (IN), on the knot (IN) and far away (OUT).
    Returns (case, the expected in-support flag per site)."""
    b = next_below(0.25)
    coords = np.array([[0.25, 0], [0, 0.25], [b, 0], [0, b], [0, 0], [0.75, 0.75], [-0.25, 0], [-b, 0]], dtype=np.float32)
    case = dict(centers=np.zeros((1, 2), dtype=np.float32), bw=np.array([0.25], dtype=np.float32), basis="wendland",
                sizes=(1,), coords=coords, w=None, v=None, rho=1.0)
    return case, np.array([0, 0, 1, 1, 1, 0, 0, 1], dtype=bool)


def searched_boundary_case(basis, bw=0.3):
    """One knot at the origin; the float32 coordinate x on the axis with x x < R2 <= x' x' for its float32 successor
    x', found by walking float32 values around sqrt(R2) of the restated R2: x is IN, x' is OUT.  Returns (case, flags)."""
    bw32 = np.float32(bw)
    rho = 1.0 if basis != "gaussian" else 1.0 / CAL[basis]
    s = float(bw32) * CAL[basis] * rho
    R2 = s * s
    x = np.float32(np.sqrt(R2))
    while float(x) * float(x) >= R2:
        x = next_below(x)
    while float(np.nextafter(x, np.float32(np.inf))) ** 2 < R2:
        x = np.nextafter(x, np.float32(np.inf))
    xo = np.nextafter(x, np.float32(np.inf))
    assert float(x) * float(x) < R2 <= float(xo) * float(xo)
    coords = np.array([[x, 0], [xo, 0], [0, x], [0, xo], [-x, 0], [0, -xo]], dtype=np.float32)
    case = dict(centers=np.zeros((1, 2), dtype=np.float32), bw=np.array([bw32]), basis=basis, sizes=(1,), coords=coords,
                w=None, v=None, rho=rho)
    return case, np.array([1, 0, 1, 0, 1, 0], dtype=bool)


# ------------------------------------------------------------------------------------------------ the tie to the model
TIE_CASES = {"wendland": "default227", "gaussian": "default227_gauss", "triangular": "default227_tri"}
TIE_S = 193
EDGE_MARGIN = 16 * 2.0 ** -24                   # a support edge within this, relative to rho, of a site: float32 may differ


def tie_sites(basis):
    """The sites of the tie to the model's own float32 basis: 193 uniform float32 points of the unit square."""
    rs = np.random.RandomState(4242 + BASES.index(basis))
    return rs.uniform(0, 1, (TIE_S, 2)).astype(np.float32)


def tie_tables(basis):
    """The knot tables of the `default227` shape as the model holds them (the oracle's uniform grid) and the sites."""
    from golden import cases
    from oracle import stdadk_oracle as orc
    cfg = cases.MODEL_CASES[TIE_CASES[basis]]
    centers, bw, _ = orc.uniform_knots(cfg["k_spatial_centers"])
    return np.asarray(centers, dtype=np.float32), np.asarray(bw, dtype=np.float32), tuple(cfg["k_spatial_centers"])


def tie_case(basis):
    centers, bw, sizes = tie_tables(basis)
    rho = 1.0 if basis != "gaussian" else 1.0 / CAL[basis]
    return dict(centers=centers, bw=bw, basis=basis, sizes=sizes, coords=tie_sites(basis), w=None, v=None, rho=rho)


def tie_edge_knots(case):
    """Knots with a site whose scaled radius is within EDGE_MARGIN (relative) of rho: left out of the tie check."""
    c, x = case["centers"].astype(np.float64), case["coords"].astype(np.float64)
    den = case["bw"].astype(np.float64) * CAL[case["basis"]]
    r = np.hypot(x[:, None, 0] - c[None, :, 0], x[:, None, 1] - c[None, :, 1]) / den[None, :]
    return (np.abs(r - case["rho"]) <= EDGE_MARGIN * case["rho"]).any(axis=0)


def tie_column_sums(phi32, case):
    """Per knot the float64 sum of a float32 phi block (S, Ks) over the pairs the CONTRACT holds in support (the mask
    matters for the Gaussian kind only, whose tail beyond rho is dropped by contract; the compact kinds are 0 there)."""
    inside = _pairs(case, np.float64)[0]
    return np.where(inside, np.asarray(phi32, dtype=np.float32).astype(np.float64), 0.0).sum(axis=0)


def tie_gap(colsum, sphi, edge):
    """The worst relative gap |colsum - SPHI| / SPHI over the knots that are not `edge` and have SPHI > 0."""
    keep = ~edge & (sphi > 0)
    return float((np.abs(colsum - sphi)[keep] / sphi[keep]).max())


def tie_oracle_gap(basis):
    """What the float32 ORACLE features show against the float64 restatement for the tie case: the figure the GPU
    test's tolerance is four times of (recorded in basis_diag_achieved.json)."""
    from oracle import stdadk_oracle as orc
    from stnf.utils import basis_diag as BD
    case = tie_case(basis)
    phi32 = orc.spatial_basis(case["coords"], case["centers"], case["bw"], basis=basis, dtype=np.float32)
    sphi = BD.basis_diag_sums_host(*call_args(case))[0][:, K_SPHI]
    return tie_gap(tie_column_sums(phi32, case), sphi, tie_edge_knots(case))


# ------------------------------------------------------------------------------------------------ the record
def measure():
    """{"worst_ratio": per basis the worst |float64 - long double| / bound over all cases, "tie_oracle_gap": per basis}."""
    from stnf.utils import basis_diag as BD
    out = {"note": "numpy float64 restatement against the long-double one, as a fraction of the comparator's bound "
                   "(worst over all cases; must stay <= 0.25), and the float32 oracle features' worst relative gap of the "
                   "per-knot column sums against the float64 restatement on the tie cases (the GPU tolerance is 4x)",
           "worst_ratio": {}, "tie_oracle_gap": {}}
    for basis in BASES:
        worst = 0.0
        for case in all_cases(basis):
            rk, rsite, aux = restate_longdouble(case)
            bad, ratio = compare(*BD.basis_diag_sums_host(*call_args(case)), rk, rsite, aux, fraction=0.25)
            assert not bad, (basis, bad[:3])
            worst = max(worst, ratio)
        out["worst_ratio"][basis] = worst
        out["tie_oracle_gap"][basis] = tie_oracle_gap(basis)
    return out


def achieved():
    with open(ACHIEVED) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "st-dadk_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    rec = measure()
    with open(ACHIEVED, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(rec)
