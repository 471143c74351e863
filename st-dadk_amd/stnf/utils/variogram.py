"""Empirical space-time semivariograms of field, prediction and residual (stdadk_variogram_f32, include/stdadk.h).

gamma(h, u) = SUM (v_a - v_b)^2 / (2 N) over the pairs a = (t, i), b = (t + u, j) whose site distance falls in the bin
of h: of the field z, of the prediction (a lower sill than the field's: over-smoothing) and of the residual z - p
(flat: the structure was captured; rising: what is left and at which range).  Pairs are counted per split and only
within one; lag 0 takes every unordered site pair once, a lag u > 0 every ordered pair, i = j included.

The sums come from the device library (`Predictor.variogram_grid`, `field_variogram` on a HIP device) or, for
`device: cpu` models and host arrays, from `variogram_sums_host`, the same contract in numpy float64.
"""
import numpy as np
import torch

VG_N, VG_SZ, VG_SP, VG_SR = 0, 1, 2, 3            # the STDADK_VG_* slots of include/stdadk.h
MAX_BINS, MAX_LAGS = 64, 16
DEFAULT_SITES = 4096


def variogram_edges(coords, n_bins=15, max_dist=None):
    """n_bins + 1 bin edges, equal-width in DISTANCE from 0 to max_dist (default: half the diagonal of the bounding box
    of `coords`), float64.  The library takes their squares, `edges * edges` in float64."""
    n_bins = int(n_bins)
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError(f"variogram: n_bins={n_bins} outside 1..{MAX_BINS}")
    if max_dist is None:
        c = np.asarray(coords, dtype=np.float64).reshape(-1, 2)
        max_dist = 0.5 * float(np.hypot(*(c.max(axis=0) - c.min(axis=0)))) if len(c) else 1.0
    max_dist = float(max_dist)
    if not max_dist > 0.0 or not np.isfinite(max_dist):
        raise ValueError(f"variogram: max_dist={max_dist} must be positive and finite (pass it when all sites coincide)")
    return np.linspace(0.0, max_dist, n_bins + 1)


def _check_edges(edges):
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    if not 2 <= len(edges) <= MAX_BINS + 1 or not edges[0] >= 0.0 or not (np.diff(edges) > 0.0).all():
        raise ValueError(f"variogram: edges must be 2..{MAX_BINS + 1} strictly increasing distances >= 0")
    e2 = edges * edges
    if not (np.diff(e2) > 0.0).all():
        raise ValueError("variogram: the squared edges are not strictly increasing in float64")
    return edges, e2


def _check_lags(time_lags):
    time_lags = int(time_lags)
    if not 1 <= time_lags <= MAX_LAGS:
        raise ValueError(f"variogram: time_lags={time_lags} outside 1..{MAX_LAGS}")
    return time_lags


def select_sites(S, sites=None):
    """The rows of the site table the variogram runs on, sorted int64: every site up to 4 096 of them, beyond that
    4 096 rows drawn without replacement by a RandomState(0) of its own (the global numpy RNG is not touched);
    'all' = every site whatever S; an index array = those rows, as given."""
    if sites is None:
        if S <= DEFAULT_SITES:
            return np.arange(S, dtype=np.int64)
        return np.sort(np.random.RandomState(0).choice(S, DEFAULT_SITES, replace=False)).astype(np.int64)
    if isinstance(sites, str):
        if sites != "all":
            raise ValueError(f"variogram: sites must be None, 'all' or an index array, got {sites!r}")
        return np.arange(S, dtype=np.int64)
    idx = np.asarray(sites).reshape(-1).astype(np.int64)
    if len(idx) and (idx.min() < 0 or idx.max() >= S):
        raise ValueError(f"variogram: site indices outside 0..{S - 1}")
    return idx


def variogram_sums_host(pred, z, code, coords, edges2, n_lags, block=256):
    """The sums of stdadk_variogram_f32 in numpy float64 (the path of `device: cpu` models): pred (T, S) float32 or
    None, z (T, S) float32 with NaN = no value, code (T, S) codes or None, coords (S, 2) float32, edges2 the squared
    edges.  Returns acc (4, n_lags, n_bins, 4) = (N, SZ, SP, SR) per split, lag and bin."""
    z = np.asarray(z, dtype=np.float32)
    T, S = z.shape
    e2 = np.asarray(edges2, dtype=np.float64)
    B, L = len(e2) - 1, int(n_lags)
    code = np.zeros((T, S), dtype=np.int64) if code is None else np.asarray(code).astype(np.int64)
    counted = np.isfinite(z) & (code >= 0) & (code <= 3)
    cc = np.where(counted, code, -1)
    zd = np.where(counted, z, 0).astype(np.float64)
    pd = None if pred is None else np.asarray(pred, dtype=np.float32).astype(np.float64)
    rd = None if pd is None else zd - pd
    x = np.asarray(coords, dtype=np.float32).astype(np.float64).reshape(S, 2)
    acc = np.zeros((4, L, B, 4))
    for i0 in range(0, S, block):
        i1 = min(S, i0 + block)
        dx, dy = x[i0:i1, None, 0] - x[None, :, 0], x[i0:i1, None, 1] - x[None, :, 1]
        d2 = dx * dx + dy * dy
        k = np.searchsorted(e2, d2, side="right")                      # edges <= d2 (a NaN sorts past the last edge)
        pair_bin = np.where((k >= 1) & (k <= B), k - 1, -1)
        upper = np.arange(i0, i1)[:, None] < np.arange(S)[None, :]
        for u in range(min(L, T)):
            pb = np.where(upper, pair_bin, -1) if u == 0 else pair_bin
            if not (pb >= 0).any():
                continue
            for t in range(T - u):
                ca, cb = cc[t, i0:i1, None], cc[t + u, None, :]
                m = (ca == cb) & (ca >= 0) & (pb >= 0)
                if not m.any():
                    continue
                slot = (np.broadcast_to(ca, m.shape)[m] * B + pb[m])
                fold = lambda w: np.bincount(slot, weights=w, minlength=4 * B).reshape(4, B)      # noqa: E731
                acc[:, u, :, VG_N] += np.bincount(slot, minlength=4 * B).reshape(4, B)
                dz = (zd[t, i0:i1, None] - zd[t + u, None, :])[m]
                acc[:, u, :, VG_SZ] += fold(dz * dz)
                if pd is not None:
                    dp = (pd[t, i0:i1, None] - pd[t + u, None, :])[m]
                    dr = (rd[t, i0:i1, None] - rd[t + u, None, :])[m]
                    acc[:, u, :, VG_SP] += fold(dp * dp)
                    acc[:, u, :, VG_SR] += fold(dr * dr)
    return acc


def variogram_curves(acc, edges, lags):
    """The curves of the sums `acc` (4, L, B, 4): count (N, int64), gamma_z, gamma_pred, gamma_resid, each (4, L, B) with
    gamma = SUM / (2 N) and NaN where N = 0 (rows in the order of the split codes: other, train, valid, test), plus
    `edges` (B + 1 distances) and `lags` (L slice offsets)."""
    acc = np.asarray(acc, dtype=np.float64)
    n = acc[..., VG_N]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = [np.where(n > 0, acc[..., k] / (2.0 * np.where(n > 0, n, 1.0)), np.nan) for k in (VG_SZ, VG_SP, VG_SR)]
    return {"count": n.astype(np.int64), "gamma_z": g[0], "gamma_pred": g[1], "gamma_resid": g[2],
            "edges": np.asarray(edges, dtype=np.float64), "lags": np.asarray(lags, dtype=np.int64)}


def device_variogram(y_pred, col, z, split, coords, edges2, n_lags, scratch=None):
    """One stdadk_variogram_f32 call on device tensors (see _native.variogram) and ONE host read: acc (4, L, B, 4) as
    a numpy array.  `scratch(name, shape, dtype)` hands out the accumulator and the workspace (default: fresh)."""
    from .. import _native as N
    nT, S = z.shape
    B, L = len(edges2) - 1, int(n_lags)
    alloc = scratch or (lambda name, shape, dtype: torch.empty(shape, device=z.device, dtype=dtype))
    acc = alloc("vg_acc", (4, L, B, 4), torch.float64)
    ws = alloc("vg_ws", (N.variogram_workspace_bytes(S, nT, B, L) // 8,), torch.float64)
    N.variogram(y_pred, col, z, split, coords, edges2, L, acc, ws)
    return acc.cpu().numpy()


def field_variogram(z, coords, code=None, edges=None, n_bins=15, max_dist=None, time_lags=1, sites=None, device=None):
    """The variogram of a field alone, e.g. of the observed data before any training: z (T, S) with NaN = no value,
    coords (S, 2), code (T, S) split codes 0..3 or None (all 0).  `edges`: the bin edges as distances (default
    variogram_edges(coords, n_bins, max_dist)); `time_lags` L: lags 0 .. L - 1; `sites`: see select_sites.
    `device`: a HIP device runs stdadk_variogram_f32 with no prediction (default: the device of `z` when it is a tensor
    on one); otherwise numpy float64 on the host.  Returns variogram_curves' dict (gamma_pred and gamma_resid are 0
    where there are pairs) plus `sites`."""
    if device is None and torch.is_tensor(z) and z.is_cuda:
        device = z.device
    host = lambda a: np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)      # noqa: E731
    z_h, c_h = host(z).astype(np.float32), host(coords).astype(np.float32)
    if z_h.ndim != 2 or c_h.shape != (z_h.shape[1], 2):
        raise ValueError(f"field_variogram: z must be (T, S) and coords (S, 2), got {z_h.shape} and {c_h.shape}")
    code_h = None if code is None else host(code).astype(np.uint8)
    if code_h is not None and code_h.shape != z_h.shape:
        raise ValueError(f"field_variogram: code has shape {code_h.shape}, z {z_h.shape}")
    L = _check_lags(time_lags)
    edges, e2 = _check_edges(variogram_edges(c_h, n_bins, max_dist) if edges is None else edges)
    idx = select_sites(z_h.shape[1], sites)
    z_s, c_s = np.ascontiguousarray(z_h[:, idx]), np.ascontiguousarray(c_h[idx])
    code_s = None if code_h is None else np.ascontiguousarray(code_h[:, idx])
    if device is not None and torch.device(device).type == "cuda":
        dev = torch.device(device)
        with torch.cuda.device(dev):
            acc = device_variogram(None, 0, torch.from_numpy(z_s).to(dev),
                                   None if code_s is None else torch.from_numpy(code_s).to(dev),
                                   torch.from_numpy(c_s).to(dev), e2, L)
    else:
        acc = variogram_sums_host(None, z_s, code_s, c_s, e2, L)
    out = variogram_curves(acc, edges, np.arange(L))
    out["sites"] = idx
    return out


VARIOGRAM_MODELS = ("exponential", "spherical", "gaussian")


def variogram_structure(model, h, range_):
    """The structure function g of a variogram model, gamma(h) = nugget + psill * g(h / range): exponential
    1 - exp(-r), spherical 1.5 r - 0.5 r^3 below the range and 1 beyond it, gaussian 1 - exp(-r^2); float64."""
    if model not in VARIOGRAM_MODELS:
        raise ValueError(f"variogram: model '{model}' must be one of {VARIOGRAM_MODELS}")
    r = np.asarray(h, dtype=np.float64) / float(range_)
    if model == "exponential":
        return 1.0 - np.exp(-r)
    if model == "gaussian":
        return 1.0 - np.exp(-(r * r))
    return np.where(r < 1.0, 1.5 * r - 0.5 * r * r * r, 1.0)


def _wls_nonneg(g, y, w):
    """min sum w (y - c0 - c g)^2 over c0, c >= 0 in closed form: the interior solution where both are >= 0, otherwise
    the better of the two boundary solutions (c0 = 0; c = 0).  Returns (c0, c, weighted residual sum)."""
    wss = lambda c0, c: float(np.sum(w * (y - c0 - c * g) ** 2))      # noqa: E731
    sw, sg, sy = float(np.sum(w)), float(np.sum(w * g)), float(np.sum(w * y))
    sgg, sgy = float(np.sum(w * g * g)), float(np.sum(w * g * y))
    det = sw * sgg - sg * sg
    if det > 0.0:
        c = (sw * sgy - sg * sy) / det
        c0 = (sy - c * sg) / sw
        if c0 >= 0.0 and c >= 0.0:
            return c0, c, wss(c0, c)
    only_c = max(sgy / sgg, 0.0) if sgg > 0.0 else 0.0
    only_c0 = max(sy / sw, 0.0)
    a, b = wss(0.0, only_c), wss(only_c0, 0.0)
    return (0.0, only_c, a) if a <= b else (only_c0, 0.0, b)


def fit_variogram(gamma, n, edges, model="exponential", ranges=None):
    """A variogram model fitted to ONE empirical curve as variogram_curves returns it: `gamma` and the pair counts `n`
    per bin, and the B + 1 bin `edges`; a bin's distance is its midpoint, bins with n == 0 or a non-finite gamma are
    skipped.  gamma(h) = nugget + psill * g(h / range) with g of `model` (variogram_structure).  Deterministic, no
    optimiser: for every candidate range of a fixed ladder -- `ranges`, default 64 log-spaced values from a quarter of
    the first bin's midpoint to twice the last edge -- the weighted least-squares (nugget, psill) >= 0 in closed form,
    weights n; the candidate with the smallest weighted residual sum wins, ties go to the smaller range.  Returns
    {"model", "nugget", "psill", "range", "wss", "bins_used"}.  Fewer than 3 usable bins, or every gamma 0: ValueError."""
    if model not in VARIOGRAM_MODELS:
        raise ValueError(f"fit_variogram: model '{model}' must be one of {VARIOGRAM_MODELS}")
    gamma = np.asarray(gamma, dtype=np.float64).reshape(-1)
    n = np.asarray(n, dtype=np.float64).reshape(-1)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    if len(edges) != len(gamma) + 1 or len(n) != len(gamma):
        raise ValueError(f"fit_variogram: {len(gamma)} bins need {len(gamma) + 1} edges and {len(gamma)} counts, got "
                         f"{len(edges)} and {len(n)}")
    use = (n > 0) & np.isfinite(gamma)
    if int(use.sum()) < 3:
        raise ValueError(f"fit_variogram: {int(use.sum())} usable bins, at least 3 are needed")
    h, y, w = (0.5 * (edges[:-1] + edges[1:]))[use], gamma[use], n[use]
    if not (y != 0.0).any():
        raise ValueError("fit_variogram: every gamma is 0 (a constant field has no variogram to fit)")
    if ranges is None:
        ranges = np.geomspace(0.25 * 0.5 * (edges[0] + edges[1]), 2.0 * edges[-1], 64)
    ranges = np.sort(np.asarray(ranges, dtype=np.float64).reshape(-1))
    if len(ranges) == 0 or not (ranges > 0.0).all() or not np.isfinite(ranges).all():
        raise ValueError("fit_variogram: the candidate ranges must be positive and finite")
    best = None
    for a in ranges:                              # ascending: a tie keeps the smaller range
        c0, c, wss = _wls_nonneg(variogram_structure(model, h, a), y, w)
        if best is None or wss < best[3]:
            best = (c0, c, float(a), wss)
    return {"model": model, "nugget": best[0], "psill": best[1], "range": best[2], "wss": best[3],
            "bins_used": int(use.sum())}
