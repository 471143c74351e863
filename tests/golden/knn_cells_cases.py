"""The cell-binned neighbour search (stdadk_knn_cells_f32, csrc/knn_cells.hip): a python restatement of its plan and the
cases that hold it to the brute-force table.  Shared by tests/test_knn_cells_cases_cpu.py (runs anywhere) and
tests/test_gpu_knn_cells.py.  Not imported by the product; no stored arrays.

CONTRACT.  For every input stdadk_knn_f32 accepts the entry assigns the same table, bit for bit; knn_host
(stnf.utils.baselines) is the statement both searches are held to, so every comparison here is knn_cases.same_table.

THE PLAN, restated (restate_cells).  G = grid_side(S): the largest g in 1 .. GMAX with OCC g g <= S.  The box is the
min and max of the coordinates of the sites with both coordinates finite; a site's column is clamp(floor((x - x0) *
(G / (x1 - x0))), 0, G - 1) in float64 (a zero extent: column 0), its row likewise; a site with a non-finite coordinate
is LOOSE (cell G G) and is met by every wave first.  Sites and targets are ordered by cell (here: stably, by index
inside a cell; the device's order inside a cell is whatever its atomics give, and the table does not depend on it).  A
wave is WAVE consecutive sorted targets of one slice.  It meets the cells of the rectangle of its lanes' cells, then one
frame of cells per ring.  After each ring a lane is done when its list holds k sources and `bound > worst` is TRUE,
where worst is its k-th d2 and bound the least, over the four sides, of the squared gap between the target and the
extreme coordinate of any site beyond that side -- LX[a0] the largest x in a column < a0, RX[a1] the smallest x in a
column > a1, LY, RY alike; one difference and one product, a gap that is not positive gives 0.  A loose target is never
done.  The wave stops when every lane is done or the rectangle is the grid.  `strict=False` turns the stop into `>=`:
the mistake the cases must catch.  The restatement counts the (target, source) pairs it meets.
"""
import numpy as np

from golden import knn_cases as kc

# the constants of csrc/knn_cells.hip (read back from the source by the CPU test)
OCC = 4                                         # KC_OCC: sites per cell the grid rule aims at
GMAX = 1024                                     # KC_GMAX: grid side at the most
WAVE = 64                                       # KC_MT: targets per wave

_EMPTY = np.uint64(0x7FF0000000000001)
_NONE = np.int64(0x7FFFFFFF)


def grid_side(S):
    g = 1
    while g < GMAX and (g + 1) * (g + 1) * OCC <= S:
        g += 1
    return g


def rule_changes(limit=4097):
    """The site counts at which grid_side changes, up to `limit`."""
    return [OCC * g * g for g in range(2, GMAX + 1) if OCC * g * g <= limit]


def _axis(v, v0, inv, G):
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((v - v0) * inv)
    return np.where(t >= G - 1, G - 1, np.where(t > 0, t, 0)).astype(np.int64)


def binning(q, coords):
    """The plan's data for targets q (M, 2) and sites coords (S, 2), float32: dict with G, the cells of sites and
    targets (G G = loose), both orders by cell, the sites' cell starts (G G + 2 entries) and the four edge arrays."""
    c, t = coords.astype(np.float64).reshape(-1, 2), q.astype(np.float64).reshape(-1, 2)
    S, G = len(c), grid_side(len(coords))
    fin = np.isfinite(c).all(axis=1)
    x0 = y0 = ix = iy = 0.0
    if fin.any():
        x0, x1, y0, y1 = c[fin, 0].min(), c[fin, 0].max(), c[fin, 1].min(), c[fin, 1].max()
        ix = G / (x1 - x0) if x1 - x0 > 0 else 0.0
        iy = G / (y1 - y0) if y1 - y0 > 0 else 0.0

    def cells(p):
        ok = np.isfinite(p).all(axis=1)
        cx, cy = _axis(p[:, 0], x0, ix, G), _axis(p[:, 1], y0, iy, G)
        return np.where(ok, cy * G + cx, G * G)
    s_cell, t_cell = cells(c), cells(t)
    s_order, t_order = np.argsort(s_cell, kind="stable"), np.argsort(t_cell, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(s_cell, minlength=G * G + 1))])
    edges = []
    for axis_, lane in ((0, s_cell % G), (1, s_cell // G)):
        lo, hi = np.full(G, np.inf), np.full(G, -np.inf)
        for i in np.nonzero(fin)[0]:
            lo[lane[i]], hi[lane[i]] = min(lo[lane[i]], c[i, axis_]), max(hi[lane[i]], c[i, axis_])
        left = np.concatenate([[-np.inf], np.maximum.accumulate(hi)[:-1]])
        right = np.concatenate([np.minimum.accumulate(lo[::-1])[::-1][1:], [np.inf]])
        edges += [left, right]
    return dict(G=G, s_cell=s_cell, t_cell=t_cell, s_order=s_order, t_order=t_order, start=start,
                LX=edges[0], RX=edges[1], LY=edges[2], RY=edges[3], box=(x0, y0, ix, iy))


def _gap2(gap):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(gap > 0, gap * gap, 0.0)


def restate_cells(case, strict=True):
    """The table by the plan: (nbr_idx (nM, M, k) int32, nbr_d2 (nM, M, k) float64, pairs met).  strict=False stops on
    `bound >= worst`."""
    q, c, src, k = case["q"], case["coords"], case["src"], case["k"]
    M, S = len(q), len(c)
    nM = 1 if src is None else len(src)
    idx = np.full((nM, M, k), -1, dtype=np.int32)
    d2 = np.full((nM, M, k), np.inf)
    if M == 0 or nM == 0:
        return idx, d2, 0
    b = binning(q, c)
    G, start = b["G"], b["start"]
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    pairs = 0
    for m in range(nM):
        flag = np.ones(S, dtype=bool) if src is None else src[m] != 0
        for w0 in range(0, M, WAVE):
            lanes = b["t_order"][w0:w0 + WAVE]                   # the wave's targets, by their index j
            L = len(lanes)
            loose = b["t_cell"][lanes] == G * G
            cx = np.where(loose, 0, b["t_cell"][lanes] % G)
            cy = np.where(loose, 0, b["t_cell"][lanes] // G)
            qx, qy = q64[lanes, 0], q64[lanes, 1]
            key = np.full((L, k), _EMPTY, dtype=np.uint64)
            ix = np.full((L, k), _NONE, dtype=np.int64)

            def walk(lo, hi):
                nonlocal key, ix, pairs
                sel = b["s_order"][lo:hi]
                sel = sel[flag[sel]]
                if not len(sel):
                    return
                pairs += L * len(sel)
                with np.errstate(invalid="ignore", over="ignore"):
                    dx, dy = qx[:, None] - c64[None, sel, 0], qy[:, None] - c64[None, sel, 1]
                    dd = dx * dx + dy * dy
                new = np.ascontiguousarray(dd).view(np.uint64).copy()
                new[np.isnan(dd)] = _EMPTY
                who = np.broadcast_to(sel[None, :].astype(np.int64), new.shape).copy()
                if case["exclude_self"]:
                    new[who == lanes[:, None]] = _EMPTY
                who[new == _EMPTY] = _NONE
                allk, alli = np.concatenate([key, new], axis=1), np.concatenate([ix, who], axis=1)
                order = np.lexsort((alli, allk), axis=1)[:, :k]     # the total order (key, index)
                key, ix = np.take_along_axis(allk, order, axis=1), np.take_along_axis(alli, order, axis=1)

            a0, a1, r0, r1 = int(cx.min()), int(cx.max()), int(cy.min()), int(cy.max())
            pa0, pa1, pr0, pr1 = 0, -1, 0, -1
            walk(start[G * G], start[G * G + 1])
            rings = 0
            while True:
                for r in range(r0, r1 + 1):
                    inner = pr0 <= r <= pr1
                    for c0, c1 in ((a0, pa0 - 1 if inner else a1), (pa1 + 1, a1 if inner else -1)):
                        if c0 <= c1:
                            walk(start[r * G + c0], start[r * G + c1 + 1])
                if (a0, a1, r0, r1) == (0, G - 1, 0, G - 1):
                    break
                worst = key[:, k - 1].copy().view(np.float64)        # NaN while the list is short
                bound = np.minimum(np.minimum(_gap2(qx - b["LX"][a0]), _gap2(b["RX"][a1] - qx)),
                                   np.minimum(_gap2(qy - b["LY"][r0]), _gap2(b["RY"][r1] - qy)))
                with np.errstate(invalid="ignore"):
                    done = ~loose & ((bound > worst) if strict else (bound >= worst))
                if done.all():
                    break
                pa0, pa1, pr0, pr1 = a0, a1, r0, r1
                a0, a1, r0, r1 = max(a0 - 1, 0), min(a1 + 1, G - 1), max(r0 - 1, 0), min(r1 + 1, G - 1)
                rings += 1
                assert rings <= G
            none = ix == _NONE
            idx[m, lanes] = np.where(none, -1, ix).astype(np.int32)
            d2[m, lanes] = np.where(none, np.inf, key.view(np.float64))
    return idx, d2, pairs


# ---- the cases -----------------------------------------------------------------------------------

SIZES_M = [63, 64, 65, 130]
SIZES_S = [1, 2] + sorted(s for g in rule_changes() for s in (g - 1, g)) + [4097]


def _case(name, q, coords, src, k, exclude_self=False):
    return dict(name=name, q=np.ascontiguousarray(q, dtype=np.float32), coords=np.ascontiguousarray(coords, dtype=np.float32),
                src=None if src is None else np.ascontiguousarray(src, dtype=np.uint8), k=k, exclude_self=exclude_self)


def lattice_edge_case():
    """80 sites on the 1/4 lattice (G = 4: every site ON a cell edge), targets at the 25 cell corners and the 16 cell
    centres: the k-th neighbour of a target ties with sources of a ring it has not met."""
    rs = np.random.RandomState(77)
    coords = kc.points(rs, 80, "lattice")
    coords[:4] = [[0, 0], [1, 0], [0, 1], [1, 1]]                     # (the box is the unit square)
    corners = np.stack(np.meshgrid(np.arange(5) / 4.0, np.arange(5) / 4.0), axis=-1).reshape(-1, 2)
    centres = np.stack(np.meshgrid((np.arange(4) + 0.5) / 4.0, (np.arange(4) + 0.5) / 4.0), axis=-1).reshape(-1, 2)
    q = np.concatenate([corners, centres, kc.points(rs, 24, "lattice")])
    assert grid_side(80) == 4 and len(q) == 65
    return _case("lattice_edges", q, coords, None, 8)


def cluster_case():
    """Five tight clusters in a 19 x 19 grid: most cells empty, a few crowded (several sites per cell)."""
    rs = np.random.RandomState(78)
    return _case("clusters", kc.points(rs, 130, "clustered"), kc.points(rs, 1500, "clustered"), None, 7)


def density_case():
    """Per-slice flags at densities 0.5 and 0.02 (fewer than k within reach: many rings), fewer than k in total, none."""
    rs = np.random.RandomState(79)
    coords = kc.points(rs, 1000, "uniform")
    src = np.zeros((4, 1000), dtype=np.uint8)
    src[0] = rs.uniform(size=1000) < 0.5
    src[1] = rs.uniform(size=1000) < 0.02
    src[2, rs.choice(1000, 5, replace=False)] = 200
    return _case("densities", kc.points(rs, 130, "uniform"), coords, src, 8)


def special_cases():
    rs = np.random.RandomState(80)
    out = [lattice_edge_case(), cluster_case(), density_case()]
    pts = kc.points(rs, 300, "uniform")
    out.append(_case("coincident", kc.points(rs, 65, "uniform"), np.repeat(pts[:1], 40, axis=0), None, 8))
    line = pts[:200].copy()
    line[:, 0] = 0.375
    out.append(_case("one_line", np.concatenate([kc.points(rs, 40, "uniform"), line[:25]]), line, None, 7))
    # targets outside the sites' box: near it, at 1e6 from it, and non-finite ones; non-finite sources too
    far = kc.points(rs, 65, "uniform") * 1.4 - 0.2
    far[:8] = [[1e6, 0.5], [-1e6, 0.5], [0.5, 1e6], [0.5, -1e6], [1e6, 1e6], [-1e6, 1e6], [3e38, 0.5], [-3e38, -3e38]]
    out.append(_case("outside", far, pts, None, 8))
    bad_q = far.copy()
    bad_q[8:14] = [[np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [0.5, -np.inf], [np.inf, np.inf], [np.nan, np.inf]]
    bad_c = pts.copy()
    bad_c[[0, 7, 150, 299]] = [[np.nan, 0.5], [np.inf, 0.5], [0.5, -np.inf], [np.inf, np.nan]]
    out.append(_case("non_finite", bad_q, bad_c, (rs.uniform(size=(2, 300)) < 0.7), 16))
    out.append(_case("only_loose_sites", far, np.full((9, 2), np.inf), None, 2))
    # leave-one-out with duplicated sites: the twin at d2 = 0 stays, self does not
    twins = np.concatenate([pts[:100], pts[:60]])
    out.append(_case("twins", twins, twins, (rs.uniform(size=(3, 160)) < 0.8), 2, exclude_self=True))
    out.append(_case("twins_all", twins, twins, None, 1, exclude_self=True))
    return out


def size_cases():
    """S = 1, 2 and just below and at every size where the grid rule changes G, up to 4097; M, k, the kind of
    coordinates and the slice count in turn."""
    out = []
    for n, S in enumerate(SIZES_S):
        M, k, kind, nM = SIZES_M[n % 4], kc.SIZES_K[n % 5], kc.KINDS[n % 3], (1, 3)[n % 2]
        c = kc.make_case(M, S, k, nM, kind, density=0.8 if nM > 1 else 1.0, seed=500 + n)
        out.append(_case(f"S{S}_M{M}_k{k}_{kind}_nM{nM}", c["q"], c["coords"], c["src"], k))
    return out


def all_cases():
    base = [dict(c, name=f"knn_cases[{i}]") for i, c in enumerate(kc.all_cases())]
    return base + special_cases() + size_cases()
