"""Basis diagnostics: what did the BASIS do?  (stdadk_basis_diag_f32, stdadk_group_norms_f32; include/stdadk.h)

Per knot: how much (training) data sits in its support -- count, weight, sum of phi and phi^2, the phi-weighted mean
of a site value such as the test MSE, the distance to the nearest weighted site; `dead` knots hold no data at all.  Per
site and level: how many knots cover it, the sum of their phi, the distance to the nearest knot; `uncovered` sites are
those to which a level contributes nothing.  And what the reference's driver reports about a trained basis
(scripts/train_st_interp.py): the group-lasso sparsity analysis of the first layer (:1662-1716), the knots' movement
(:1900-1909, :2590-2596), the out-of-domain count (:1789), per-level bandwidth statistics (:2347-2361) and
`basis_info.npz` (:2570-2596).

The accumulators come from the device library (`Predictor.basis_diagnostics`) or, for `device: cpu` models and host
arrays, from `basis_diag_sums_host` / `group_sumsq_host`, the same contracts in numpy float64.
"""
import math
import os

import numpy as np
import torch

# the STDADK_BD_* slots of include/stdadk.h
K_N, K_W, K_SPHI, K_SPHI2, K_SV, K_WV, K_NEAR2, KNOT_SLOTS = 0, 1, 2, 3, 4, 5, 6, 7
S_COVER, S_SPHI, S_NEAR2, SITE_SLOTS = 0, 1, 2, 3
MAX_LEVELS = 8
CAL = {"wendland": 1.0, "gaussian": 0.223477, "triangular": 0.654714}
BASIS_INFO_KEYS = ("spatial_centers_init", "spatial_centers_final", "spatial_bandwidths_init", "spatial_bandwidths_final",
                   "temporal_centers_init", "temporal_centers_final", "temporal_bandwidths_init",
                   "temporal_bandwidths_final")


def default_rho(basis):
    """The support radius in units of the scaled radius r: 1 for the compact kinds, their exact support; 1 / cal for
    the Gaussian, i.e. distance < bandwidth (phi > exp(-0.5 / cal^2), about e^-10)."""
    return 1.0 if basis in ("wendland", "triangular") else 1.0 / CAL[basis]


def _check(centers, bw, basis, level_sizes, coords, w, v, rho):
    if basis not in CAL:
        raise ValueError(f"basis_diag: unknown basis {basis!r}")
    c = np.asarray(centers, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    b = np.asarray(bw, dtype=np.float32).reshape(-1).astype(np.float64)
    x = np.asarray(coords, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    sizes = [int(n) for n in level_sizes]
    if not 1 <= len(sizes) <= MAX_LEVELS or min(sizes) < 0 or sum(sizes) != len(c) or len(b) != len(c):
        raise ValueError(f"basis_diag: level sizes {sizes} must be 1..{MAX_LEVELS} counts >= 0 summing to Ks={len(c)}")
    rho = default_rho(basis) if rho is None else float(rho)
    if not (np.isfinite(rho) and rho > 0.0):
        raise ValueError(f"basis_diag: rho={rho} must be finite and > 0")
    w = np.ones(len(x)) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    v = None if v is None else np.asarray(v, dtype=np.float64).reshape(-1)
    if len(w) != len(x) or (v is not None and len(v) != len(x)):
        raise ValueError("basis_diag: w and v must have one entry per site")
    den = b * CAL[basis]
    s = den * rho
    return c, den, s * s, sizes, x, w, v


def phi_f64(r, basis):
    """phi(r) in float64 with the operations of the contract (csrc/basis.h's formulas, every product rounded once)."""
    r = np.asarray(r, dtype=np.float64)
    if basis == "wendland":
        r = np.minimum(r, 1.0)
        om = 1.0 - r
        om2 = om * om
        return (om2 * om2 * om2) * ((35.0 * r + 18.0) * r + 3.0) / 3.0
    if basis == "gaussian":
        return np.exp(-0.5 * r * r)
    return np.maximum(1.0 - r, 0.0)


def basis_diag_sums_host(centers, bw, basis, level_sizes, coords, w=None, v=None, rho=None, block=512):
    """The accumulators of stdadk_basis_diag_f32 in numpy float64 (the path of `device: cpu` models): centers (Ks, 2),
    bw (Ks,) float32 bandwidths, level_sizes the knot counts per level, coords (S, 2) float32, w / v (S,) or None.
    Returns knot_acc (Ks, 7) and site_acc (S, n_levels, 3).  Sites are walked in blocks of `block`."""
    c, den, R2, sizes, x, w, v = _check(centers, bw, basis, level_sizes, coords, w, v, rho)
    Ks, S, L = len(c), len(x), len(sizes)
    knot, site = np.zeros((Ks, KNOT_SLOTS)), np.zeros((S, L, SITE_SLOTS))
    knot[:, K_NEAR2] = np.inf
    site[:, :, S_NEAR2] = np.inf
    off = np.concatenate([[0], np.cumsum(sizes)])
    counted = np.isfinite(w) & (w > 0.0)
    wc = np.where(counted, w, 0.0)
    vfin = np.isfinite(v) if v is not None else np.zeros(S, dtype=bool)
    vz = np.where(vfin, v, 0.0) if v is not None else np.zeros(S)
    for i0 in range(0, S, block):
        i1 = min(S, i0 + block)
        dx, dy = x[i0:i1, None, 0] - c[None, :, 0], x[i0:i1, None, 1] - c[None, :, 1]
        d2 = dx * dx + dy * dy                                            # (sites, knots)
        inside = d2 < R2[None, :]
        with np.errstate(invalid="ignore"):
            phi = np.where(inside, phi_f64(np.sqrt(d2) / den[None, :], basis), 0.0)
        d2m = np.where(np.isnan(d2), np.inf, d2)
        cm = counted[i0:i1, None]
        t = wc[i0:i1, None] * phi
        hit = inside & cm
        knot[:, K_N] += hit.sum(axis=0)
        knot[:, K_W] += np.where(hit, wc[i0:i1, None], 0.0).sum(axis=0)
        knot[:, K_SPHI] += t.sum(axis=0)
        knot[:, K_SPHI2] += (t * phi).sum(axis=0)
        knot[:, K_SV] += np.where(vfin[i0:i1, None], t * vz[i0:i1, None], 0.0).sum(axis=0)
        knot[:, K_WV] += np.where(vfin[i0:i1, None], t, 0.0).sum(axis=0)
        if Ks:
            knot[:, K_NEAR2] = np.minimum(knot[:, K_NEAR2], np.where(cm, d2m, np.inf).min(axis=0, initial=np.inf))
        for l in range(L):
            a, b = off[l], off[l + 1]
            site[i0:i1, l, S_COVER] = inside[:, a:b].sum(axis=1)
            site[i0:i1, l, S_SPHI] = phi[:, a:b].sum(axis=1)
            site[i0:i1, l, S_NEAR2] = d2m[:, a:b].min(axis=1, initial=np.inf)
    return knot, site


def _phi_scalar(r, basis):
    """phi_f64 on one Python float: the same IEEE operations."""
    if basis == "wendland":
        r = r if r < 1.0 else 1.0
        om = 1.0 - r
        om2 = om * om
        return (om2 * om2 * om2) * ((35.0 * r + 18.0) * r + 3.0) / 3.0
    if basis == "gaussian":
        return math.exp(-0.5 * r * r)
    om = 1.0 - r
    return om if om > 0.0 else 0.0


def restate_exact(centers, bw, basis, level_sizes, coords, w=None, v=None, rho=None):
    """basis_diag_sums_host as plain loops over Python floats, one pair at a time, a knot's sites in site order and a
    site's knots in knot order: the slow statement of the contract, for small shapes."""
    c, den, R2, sizes, x, w, v = _check(centers, bw, basis, level_sizes, coords, w, v, rho)
    Ks, S, L = len(c), len(x), len(sizes)
    inf = float("inf")
    knot = [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, inf] for _ in range(Ks)]
    site = [[[0.0, 0.0, inf] for _ in range(L)] for _ in range(S)]
    level = np.repeat(np.arange(L), sizes).tolist()
    c, den, R2, x, w = c.tolist(), den.tolist(), R2.tolist(), x.tolist(), w.tolist()
    v = None if v is None else v.tolist()
    for i in range(S):
        xi, yi, wi = x[i][0], x[i][1], w[i]
        counted = math.isfinite(wi) and wi > 0.0
        has_v = v is not None and math.isfinite(v[i])
        rows = site[i]
        for k in range(Ks):
            dx, dy = xi - c[k][0], yi - c[k][1]
            d2 = dx * dx + dy * dy
            inside = d2 < R2[k]
            phi = _phi_scalar(math.sqrt(d2) / den[k], basis) if inside else 0.0
            row = rows[level[k]]
            if d2 < row[S_NEAR2]:
                row[S_NEAR2] = d2
            if inside:
                row[S_COVER] += 1.0
                row[S_SPHI] += phi
            if not counted:
                continue
            kr = knot[k]
            if d2 < kr[K_NEAR2]:
                kr[K_NEAR2] = d2
            if inside:
                t = wi * phi
                kr[K_N] += 1.0
                kr[K_W] += wi
                kr[K_SPHI] += t
                kr[K_SPHI2] += t * phi
                if has_v:
                    kr[K_SV] += t * v[i]
                    kr[K_WV] += t
    return np.asarray(knot, dtype=np.float64).reshape(Ks, KNOT_SLOTS), \
        np.asarray(site, dtype=np.float64).reshape(S, L, SITE_SLOTS)


def group_sumsq_host(weight, col0, n):
    """stdadk_group_norms_f32 in numpy float64: `weight` the first Linear's (H, D) weight; returns the (n,) sums of
    squares of the columns col0 .. col0 + n - 1, each weight squared in double."""
    blk = np.asarray(weight, dtype=np.float32)[:, col0:col0 + n].astype(np.float64)
    return (blk * blk).sum(axis=0)


# ---- host summaries ---------------------------------------------------------------------------

def sparsity_summary(sumsq, ratio=1e-2):
    """The reference's sparsity analysis (scripts/train_st_interp.py:1679-1716) from the groups' sums of squares:
    norms, `inactive = norm < ratio * max(norm)` (threshold 0 when the largest norm is 0: nothing is inactive), the
    counts, min / max / median / mean, the P10 / 25 / 50 / 75 / 90 line and the <0.1 % / <1 % / <10 % of max counts."""
    norms = np.sqrt(np.asarray(sumsq, dtype=np.float64).reshape(-1))
    top = float(norms.max()) if len(norms) else 0.0
    threshold = float(ratio) * top if top > 0 else 0.0
    inactive = norms < threshold
    pct = (10, 25, 50, 75, 90)
    some = len(norms) > 0
    return {"norms": norms, "inactive": inactive, "threshold": threshold, "n_inactive": int(inactive.sum()),
            "n_active": int((~inactive).sum()), "norm_min": float(norms.min()) if some else np.nan, "norm_max": top,
            "norm_median": float(np.median(norms)) if some else np.nan,
            "norm_mean": float(norms.mean()) if some else np.nan, "percentiles": np.asarray(pct),
            "percentile_values": np.percentile(norms, pct) if some else np.full(len(pct), np.nan),
            "small_counts": np.asarray([int((norms < f * top).sum()) for f in (1e-3, 1e-2, 1e-1)])}


def movement_summary(centers_init, centers_final, inactive=None):
    """|final - init| per knot and its mean / max / median / min, over the ACTIVE knots when a mask exists, as the
    reference's figure does (scripts/train_st_interp.py:1900-1909; :2590-2596 prints mean / max / min); 0 when no
    knot is left."""
    a, b = np.asarray(centers_init, dtype=np.float64), np.asarray(centers_final, dtype=np.float64)
    move = np.linalg.norm(b - a, axis=1)
    sel = move if inactive is None else move[~np.asarray(inactive, dtype=bool)]
    stat = lambda f: float(f(sel)) if len(sel) else 0.0      # noqa: E731
    return {"movement": move, "movement_mean": stat(np.mean), "movement_max": stat(np.max),
            "movement_median": stat(np.median), "movement_min": stat(np.min)}


def path_length(centers_init, history, centers_final):
    """The length of every knot's path init -> the snapshots of `history` (train_model's basis_centers_history: (epoch,
    centres) pairs, or plain arrays) in order -> final: (Ks,) float64.  Never below the movement."""
    pts = [np.asarray(centers_init, dtype=np.float64)]
    for h in history or ():
        pts.append(np.asarray(h[1] if isinstance(h, (tuple, list)) else h, dtype=np.float64))
    pts.append(np.asarray(centers_final, dtype=np.float64))
    return sum((np.linalg.norm(q - p, axis=1) for p, q in zip(pts[:-1], pts[1:])), np.zeros(len(pts[0])))


def out_of_domain(centers):
    """The count of centres outside the unit square (scripts/train_st_interp.py:1789) and their mask."""
    c = np.asarray(centers)
    mask = ((c < 0) | (c > 1)).any(axis=1)
    return int(mask.sum()), mask


def level_bandwidth_stats(bw, level_sizes):
    """Per level the bandwidths' mean / std / min / max (scripts/train_st_interp.py:2356-2361: numpy's population
    std), each (n_levels,); NaN for a level without knots."""
    bw = np.asarray(bw, dtype=np.float64).reshape(-1)
    out = {k: np.full(len(level_sizes), np.nan) for k in ("level_bw_mean", "level_bw_std", "level_bw_min", "level_bw_max")}
    o = 0
    for l, n in enumerate(level_sizes):
        part = bw[o:o + n]
        o += n
        if n:
            out["level_bw_mean"][l], out["level_bw_std"][l] = part.mean(), part.std()
            out["level_bw_min"][l], out["level_bw_max"][l] = part.min(), part.max()
    return out


def temporal_support(t_centers, t_bw, t_values, t_weights):
    """Per temporal knot the sum over the times of w_t psi(t), psi = exp(-0.5 ((t - c) / bw)^2), in float64 on the host
    (Kt x T is tiny): (Kt,)."""
    c, b = np.asarray(t_centers, dtype=np.float64).reshape(-1), np.asarray(t_bw, dtype=np.float64).reshape(-1)
    t, w = np.asarray(t_values, dtype=np.float64).reshape(-1), np.asarray(t_weights, dtype=np.float64).reshape(-1)
    s = (t[None, :] - c[:, None]) / b[:, None]
    return (w[None, :] * np.exp(-0.5 * s * s)).sum(axis=1)


def summarize(knot_acc, site_acc, level_sizes, centers, bw, sumsq=None, ratio=1e-2, centers_init=None, history=None):
    """The diagnostics dict from ONE read of the accumulators (host arrays): the per-knot slots under their names
    (knot_count, knot_weight, knot_sphi, knot_sphi2, knot_value = SV / WV, knot_nearest = sqrt(NEAR2)), `dead`
    (N == 0), `knot_level`; per site and level site_cover, site_sphi, site_nearest, `uncovered` (COVER == 0), each
    (S, n_levels); per level level_dead, level_uncovered and the bandwidth statistics; out_of_domain; with `sumsq` (the
    spatial groups' sums of squares) the sparsity analysis under `sparsity_*` and `inactive`; with `centers_init` the
    movement (over active knots when a mask exists) and the path length through `history`."""
    knot_acc, site_acc = np.asarray(knot_acc, dtype=np.float64), np.asarray(site_acc, dtype=np.float64)
    sizes = [int(n) for n in level_sizes]
    level = np.repeat(np.arange(len(sizes)), sizes)
    with np.errstate(divide="ignore", invalid="ignore"):
        value = np.where(knot_acc[:, K_WV] > 0, knot_acc[:, K_SV] / np.where(knot_acc[:, K_WV] > 0, knot_acc[:, K_WV], 1.0),
                         np.nan)
    dead = knot_acc[:, K_N] == 0
    uncovered = site_acc[:, :, S_COVER] == 0
    out = {"level_sizes": np.asarray(sizes, dtype=np.int64), "knot_level": level,
           "knot_count": knot_acc[:, K_N].astype(np.int64), "knot_weight": knot_acc[:, K_W],
           "knot_sphi": knot_acc[:, K_SPHI], "knot_sphi2": knot_acc[:, K_SPHI2], "knot_value": value,
           "knot_nearest": np.sqrt(knot_acc[:, K_NEAR2]), "dead": dead, "n_dead": int(dead.sum()),
           "site_cover": site_acc[:, :, S_COVER].astype(np.int64), "site_sphi": site_acc[:, :, S_SPHI],
           "site_nearest": np.sqrt(site_acc[:, :, S_NEAR2]), "uncovered": uncovered,
           "level_dead": np.asarray([int(dead[level == l].sum()) for l in range(len(sizes))], dtype=np.int64),
           "level_uncovered": uncovered.sum(axis=0).astype(np.int64)}
    out.update(level_bandwidth_stats(bw, sizes))
    out["out_of_domain"], out["out_of_domain_mask"] = out_of_domain(centers)
    inactive = None
    if sumsq is not None:
        sp = sparsity_summary(sumsq, ratio)
        inactive = out["inactive"] = sp.pop("inactive")
        out.update({f"sparsity_{k}": val for k, val in sp.items()})
    if centers_init is not None:
        out.update(movement_summary(centers_init, centers, inactive))
        out["path_length"] = path_length(centers_init, history, centers)
    return out


def _first_weight(model):
    return model._body[0].weight.detach()


@torch.no_grad()
def basis_diagnostics(model, coords, train_mask=None, config=None, model_initial=None, history=None, site_value=None,
                      rho=None, predictor=None):
    """The basis diagnostics of a model at the sites `coords` (S, 2): the site weights are `train_mask.sum(0)` (the
    training observations per site; all 1 without a mask), `site_value` (S,) e.g. the per-site test MSE.  A model on a
    HIP device goes through `Predictor.basis_diagnostics` (two library calls, one host read), any other through the
    numpy float64 statements of the same contracts.  `config`: `sparsity_threshold_ratio` (1e-2); the sparsity
    analysis is made whatever the penalty was.  `model_initial` (the model before training) gives movement and path
    length (`history`: train_model's basis_centers_history).  Returns summarize()'s dict plus `rho`, `site_weight`,
    and the temporal knots' `temporal_support` (sum over the times of w_t psi, w_t the training observations per
    time; float64 on the host) and `temporal_sparsity_*`.  `predictor`: reuse one of the model's."""
    config = config or {}
    sb, tb = model.spatial_basis, model.temporal_basis
    dev = next(model.parameters()).device
    host = lambda a: np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)      # noqa: E731
    c_h = host(coords).astype(np.float32).reshape(-1, 2)
    S = len(c_h)
    mask = None if train_mask is None else host(train_mask).astype(bool)
    if mask is not None and (mask.ndim != 2 or mask.shape[1] != S):
        raise ValueError(f"basis_diagnostics: train_mask must be (T, S) with S={S}, got {mask.shape}")
    w = None if mask is None else mask.sum(axis=0).astype(np.float64)
    v = None if site_value is None else host(site_value).astype(np.float64).reshape(-1)
    basis = model.spatial_basis_function
    rho = default_rho(basis) if rho is None else float(rho)
    sizes = list(sb.n_centers)
    p, Ks, Kt = model.p, model.k_spatial, model.k_temporal
    if dev.type == "cuda":
        from ..engine import Predictor
        with torch.cuda.device(dev):
            raw = (predictor or Predictor(model)).basis_diagnostics(
                torch.from_numpy(c_h).to(dev), None if w is None else torch.from_numpy(w).to(dev),
                None if v is None else torch.from_numpy(v).to(dev), rho)
        knot, site, sumsq, centers, bw = (raw[k] for k in ("knot_acc", "site_acc", "sumsq", "centers", "bandwidths"))
    else:
        centers, bw = host(sb.centers).astype(np.float32), host(sb.bandwidths).astype(np.float32)
        knot, site = basis_diag_sums_host(centers, bw, basis, sizes, c_h, w, v, rho)
        sumsq = group_sumsq_host(host(_first_weight(model)), p, Ks + Kt)
    ratio = float(config.get("sparsity_threshold_ratio", 1e-2))
    init = None if model_initial is None else host(model_initial.spatial_basis.centers).astype(np.float32)
    out = summarize(knot, site, sizes, centers, bw, sumsq[:Ks], ratio, init, history)
    out["rho"], out["site_weight"] = rho, np.ones(S) if w is None else w
    tsp = sparsity_summary(sumsq[Ks:], ratio)
    out.update({f"temporal_sparsity_{k}": val for k, val in tsp.items()})
    if mask is not None:
        T = mask.shape[0]
        tv = np.arange(T, dtype=np.float64) / (T - 1) if T > 1 else np.zeros(1)
        out["temporal_support"] = temporal_support(host(tb.centers), host(tb.bandwidths), tv, mask.sum(axis=1))
    return out


def save_basis_info_npz(path, diag, model_initial, model):
    """Writes the reference's `basis_info.npz` (scripts/train_st_interp.py:2575-2586: the eight keys
    spatial_centers_init ... temporal_bandwidths_final) plus every entry of the diagnostics dict `diag` (or None) as
    `diag/<name>`, to `path` (a directory: `<path>/basis_info.npz`); returns the file's path."""
    host = lambda a: a.detach().cpu().numpy()      # noqa: E731
    arrs = {}
    for tag, m in (("init", model_initial), ("final", model)):
        arrs[f"spatial_centers_{tag}"] = host(m.spatial_basis.centers)
        arrs[f"spatial_bandwidths_{tag}"] = host(m.spatial_basis.bandwidths)
        arrs[f"temporal_centers_{tag}"] = host(m.temporal_basis.centers)
        arrs[f"temporal_bandwidths_{tag}"] = host(m.temporal_basis.bandwidths)
    for k, val in (diag or {}).items():
        arrs[f"diag/{k}"] = np.asarray(val)
    path = str(path)
    if not path.endswith(".npz"):
        os.makedirs(path, exist_ok=True)
        path = os.path.join(path, "basis_info.npz")
    np.savez(path, **arrs)
    return path
